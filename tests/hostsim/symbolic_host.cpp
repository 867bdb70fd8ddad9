// TEST INFRASTRUCTURE -- crafter_symbolic's body (csrc/symbolic.hpp) on the CPU through WaveHost (see wave_host.hpp).
#include "walks.hpp"   // (launch_plan.hpp's LaunchPlan::maps_in_lds: the chooser between the two object paths, as the library's)
#include "../../crafter_amd/csrc/symbolic.hpp"

using namespace crafter;

extern "C" {

int hostsim_symbolic_map_is_state(const Config* cfg) { return launch_plan(*cfg, false).maps_in_lds ? 0 : 1; }

// cfg / tb / st: a HostSimEnv's.  local: [N][2][gw][gh] bytes or null, stats: [N][n_items + 4] floats or null.
int hostsim_symbolic(const Config* cfg, const TablePtrs* tb, const StatePtrs* st, const uint8_t* mask, uint8_t* local, float* stats) {
  FakeLds strip(symbolic_strip_bytes(*cfg) / 4 * 4);
  const bool map_is_state = !launch_plan(*cfg, false).maps_in_lds;
  // one env beyond the batch, as the last workgroup's spare waves: must return without touching anything
  for (int env = 0; env < cfg->num_envs + 1; env++) {
    WaveHost w;
    uint8_t* lds = strip.fresh();
    if (map_is_state)
      symbolic_body<WaveHost, 1>(w, lds, env, *cfg, *tb, *st, mask, local, stats);
    else
      symbolic_body<WaveHost, 0>(w, lds, env, *cfg, *tb, *st, mask, local, stats);
  }
  return 0;
}

}  // extern "C"
