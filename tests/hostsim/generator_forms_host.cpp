// TEST INFRASTRUCTURE -- the three ways the library makes the world of one (seed lane, episode), on the CPU through WaveHost
// (see wave_host.hpp), each in freshly poisoned "LDS" of exactly the size its kernel is launched with (but the seed stage's):
//   hostsim_forms_reset     Env.reset into the env's row: reset_body (crafter_reset_kernel, the requeue kernels)
//   hostsim_forms_fused     the fused form into a pool entry: gen_body (what crafter_reset_kernel appends through gen_one)
//   hostsim_forms_pipeline  the world pool's three kernels into a pool entry: gen_seed_body, gen_classify_body, gen_resolve_body
// The pool forms write entry (episode & 1) * num_envs + env and stamp it with batch sequence 1; a request whose world the entry
// already holds is a duplicate to them (gen_done_already): the caller empties the entry's header between two forms.
#include <string.h>

#include <vector>

#include "wave_host.hpp"
#include "../../crafter_amd/csrc/env_kernels.hpp"
#include "../../crafter_amd/csrc/launch_plan.hpp"

using namespace crafter;

namespace {
struct ExactLds {   // (its own allocation per body: a sanitised build sees every byte past it)
  std::vector<uint8_t> bytes;
  explicit ExactLds(int n) : bytes((size_t)n, 0xCD) {}
  uint8_t* data() { return bytes.data(); }
};
}  // namespace

extern "C" {

// Returns the episode the env is now in (rec.episode + 1 as it stood).
int hostsim_forms_reset(const Config* cfg, const TablePtrs* tb, const StatePtrs* st, int env, uint8_t* obs) {
  ExactLds lds(launch_plan(*cfg, is_default_rules(*tb->rules)).reset_lds);
  WaveHost w;
  return reset_body(w, lds.data(), env, *cfg, *tb, *st, obs, -1);
}

void hostsim_forms_fused(const Config* cfg, const TablePtrs* tb, const StatePtrs* st, int env, int episode) {
  ExactLds lds(launch_plan(*cfg, is_default_rules(*tb->rules)).reset_lds);
  WaveHost w;
  gen_body(w, lds.data(), env, episode, 1u, *cfg, *tb, *st);
}

void hostsim_forms_pipeline(const Config* cfg, const TablePtrs* tb, const StatePtrs* st, int env, int episode) {
  WaveHost w;
  {
    ExactLds lds(align16(4 * MT_N) + WG_LDS_BYTES);   // (kGenSeedLds, and room for WorldGen's whole block behind the MT state)
    gen_seed_body(w, lds.data(), env, episode, *cfg, *tb, *st);
  }
  for (int part = 0, parts = gen_classify_parts(*cfg); part < parts; part++) {
    ExactLds lds(gen_classify_lds_bytes(*cfg));
    gen_classify_body(w, lds.data(), env, episode, part, parts, *cfg, *tb, *st);
  }
  ExactLds lds(gen_resolve_layout(*cfg).total);
  gen_resolve_body(w, lds.data(), env, episode, 1u, *cfg, *tb, *st);
}

}  // extern "C"
