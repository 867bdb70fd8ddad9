// TEST INFRASTRUCTURE -- crafter_reset_worlds on the CPU through WaveHost (see wave_host.hpp): the host-side refusals of the
// entry point and the kernel's body (csrc/env_worlds.hpp reset_world_body), one env after the other, each in freshly poisoned
// "LDS" of exactly the size the library launches with (launch_plan's reset_lds).  The reset kernel's pool tail is the library's
// own (csrc/entry_kernels.hpp reset_pool_tail) and is not played here: the harness runs with the world pool off.
#include <string.h>

#include <vector>

#include "wave_host.hpp"
#include "../../crafter_amd/csrc/env_worlds.hpp"
#include "../../crafter_amd/csrc/launch_plan.hpp"

using namespace crafter;

extern "C" {

// Returns 0, or -1 for what the library refuses on the host.
int hostsim_reset_worlds(const Config* cfg, const TablePtrs* tb, const StatePtrs* st, const uint8_t* mask, const int32_t* world_id,
                         const uint8_t* bank_mat, const Obj* bank_objs, const int32_t* bank_nobj, const int32_t* bank_inv, int32_t n_worlds,
                         int32_t bank_max_objects, uint8_t* obs) {
  if (!bank_mat || !bank_objs || !bank_nobj || n_worlds < 1 || bank_max_objects < 0 || ((uintptr_t)bank_objs & 15u) != 0) return -1;
  WorldBank bank;
  bank.world_id = world_id;
  bank.mat = bank_mat;
  bank.objs = bank_objs;
  bank.nobj = bank_nobj;
  bank.inv = bank_inv;
  bank.n_worlds = n_worlds;
  bank.max_objects = bank_max_objects;
  const int lds_bytes = launch_plan(*cfg, is_default_rules(*tb->rules)).reset_lds;
  for (int env = 0; env < cfg->num_envs; env++) {
    if (mask && !mask[env]) continue;
    std::vector<uint8_t> lds((size_t)lds_bytes, 0xCD);   // (its own allocation per env: a sanitised build sees every byte past it)
    WaveHost w;
    reset_world_body(w, lds.data(), env, *cfg, *tb, *st, bank, obs);
  }
  return 0;
}

}  // extern "C"
