// TEST INFRASTRUCTURE -- crafter_navigate's bodies (csrc/navigate.hpp) on the CPU through WaveHost (see wave_host.hpp).
#include <string.h>

#include <vector>

#include "wave_host.hpp"
#include "../../crafter_amd/csrc/launch_plan.hpp"   // LaunchPlan::maps_in_lds: the chooser between the two object paths, as the library's
#include "../../crafter_amd/csrc/navigate.hpp"

using namespace crafter;

extern "C" {

int hostsim_navigate_map_is_state(const Config* cfg) { return launch_plan(*cfg, false).maps_in_lds ? 0 : 1; }
int hostsim_navigate_in_registers(const Config* cfg) { return nav_in_registers(*cfg) ? 1 : 0; }

// cfg / tb / st: a HostSimEnv's.  targets: k class sets; dist, first: [N][k]; facing: [N][k] or null.  force_map: -1 the object
// path the library would take, 0 / 1 that one (a world whose slot map is state keeps both views of its objects).
// -> 0, or what crafter_navigate refuses: the number of nav_check's reason, 6 for a null dist / first, 7 for boards beyond the LDS.
int hostsim_navigate(const Config* cfg, const TablePtrs* tb, const StatePtrs* st, const uint8_t* mask, const uint32_t* targets, int32_t k,
                     uint32_t passable, int32_t* dist, int32_t* first, uint8_t* facing, int force_map) {
  if (const int why = nav_check(tb->rules->n_materials, targets, k, passable)) return why;
  if (!dist || !first) return 6;
  NavQuery q;
  memset(&q, 0, sizeof(q));
  memcpy(q.targets, targets, sizeof(uint32_t) * (size_t)k);
  q.passable = passable;
  q.k = k;
  const bool map_is_state = force_map < 0 ? !launch_plan(*cfg, false).maps_in_lds : force_map != 0;
  if (!nav_in_registers(*cfg) && nav_lds_bytes(*cfg) > (size_t)kNavMaxLds) return 7;
  // one env beyond the batch, as the last workgroup's spare waves: must return without touching anything
  for (int env = 0; env < cfg->num_envs + 1; env++) {
    WaveHost w;
    if (nav_in_registers(*cfg)) {
      uint32_t strip[kNavStripWords];
      memset(strip, 0xA5, sizeof(strip));   // (LDS comes uninitialised)
      if (map_is_state)
        navigate_body<WaveHost, 1>(w, strip, env, *cfg, *tb, *st, mask, q, dist, first, facing);
      else
        navigate_body<WaveHost, 0>(w, strip, env, *cfg, *tb, *st, mask, q, dist, first, facing);
    } else {
      std::vector<uint32_t> lds(nav_lds_bytes(*cfg) / 4, 0xA5A5A5A5u);   // exactly the bytes the kernel is given
      if (map_is_state)
        navigate_lds_body<WaveHost, 1>(w, lds.data(), env, *cfg, *tb, *st, mask, q, dist, first, facing);
      else
        navigate_lds_body<WaveHost, 0>(w, lds.data(), env, *cfg, *tb, *st, mask, q, dist, first, facing);
    }
  }
  return 0;
}

const char* hostsim_navigate_error(int reason) { return reason == 6 ? "dist or first is null" : reason == 7 ? "the area's boards exceed the LDS" : nav_error_text(reason); }

}  // extern "C"
