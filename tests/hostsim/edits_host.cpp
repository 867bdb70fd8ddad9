// TEST INFRASTRUCTURE -- crafter_edit_envs on the CPU through WaveHost (see wave_host.hpp): the host-side refusals of the entry
// point, the index check's body (csrc/crafter_rollout_subset.hpp) and the kernel's body (csrc/env_edit.hpp edit_body), one named
// env after the other, each in freshly poisoned "LDS" of exactly the size the library launches with (edit_layout's total).
#include <string.h>

#include <vector>

#include "walks.hpp"
#include "../../crafter_amd/csrc/crafter_rollout_subset.hpp"
#include "../../crafter_amd/csrc/env_edit.hpp"

using namespace crafter;

extern "C" {

int hostsim_edit_lds_bytes(const Config* cfg) { return edit_layout(*cfg).total; }

// mark: int32[num_envs + 1] kept by the caller between calls (the handle's marks, then the verdict word); stamp: the call's
// number; next_step: int32[num_envs] or null (an ordered handle's hint).  Returns the verdict (0: edited, 1: refused) or -1 for
// what the library refuses on the host.
int hostsim_edit_envs(const Config* cfg, const TablePtrs* tb, const StatePtrs* st, const int32_t* idx, int n, const int32_t* ops,
                      int ops_per_env, int32_t* mark, int32_t stamp, int32_t* next_step) {
  if (n < 0 || n > cfg->num_envs) return -1;
  if (n == 0) return 0;
  if (!idx || !ops || ops_per_env < 1 || ((uintptr_t)ops & 15u) != 0) return -1;
  std::vector<int32_t> row_of((size_t)cfg->num_envs, -1);
  int flags[2];
  RolloutEnvsCheck c;
  c.idx = idx; c.n = n; c.stamp = stamp; c.mark = mark; c.verdict = mark + cfg->num_envs;
  c.rec = (EnvRec*)st->rec; c.rows = cfg->num_envs; c.row_of = row_of.data();
  rollout_envs_check_body(CheckThreadsHost{}, c, flags);
  const int lds_bytes = edit_layout(*cfg).total;
  for (int b = 0; b < n; b++) {   // workgroup b of the launch
    const int env = step_envs_env(idx, c.verdict, b);
    if (env < 0) continue;
    std::vector<uint8_t> lds((size_t)lds_bytes, 0xCD);   // (its own allocation per env: a sanitised build sees every byte past it)
    WaveHost w;
    edit_body(w, lds.data(), env, *cfg, *tb, *st, ops + (size_t)b * (size_t)ops_per_env * kEditWords, ops_per_env, next_step);
  }
  return *c.verdict;
}

}  // extern "C"
