// TEST INFRASTRUCTURE -- crafter_audit's body (csrc/audit.hpp) on the CPU through WaveHost (see wave_host.hpp).
#include <string.h>

#include <vector>

#include "wave_host.hpp"
#include "../../crafter_amd/csrc/audit.hpp"

using namespace crafter;

// WaveHost plus the primitives audit.hpp adds to the wave policy (wave_gfx950.hpp lds_min, lds_fetch_or).
struct AuditWaveHost : WaveHost {
  void lds_min(uint32_t* p, uint32_t v) const {
    if (v < *p) *p = v;
  }
  uint32_t lds_fetch_or(uint32_t* p, uint32_t v) const {
    const uint32_t old = *p;
    *p |= v;
    return old;
  }
};

extern "C" {

// cfg / tb / st: a HostSimEnv's.  map: objmap is state (hostsim_slot_map_derived() == 0).  flags: [N]; detail: [N][4].
int hostsim_audit(const Config* cfg, const TablePtrs* tb, const StatePtrs* st, int map, const uint8_t* mask, int32_t* flags, int32_t* detail) {
  if (!flags || !detail) return 1;   // what crafter_audit refuses
  const size_t words = audit_lds_words(*cfg);
  if (words * 4 > (size_t)kAuditMaxLds) return 1;
  // the "LDS" in a buffer of exactly its size, filled with another pattern for every env: the body must clear what it reads.
  // One env beyond the batch, as a grid rounded up would bring: must return without touching anything
  for (int env = 0; env < cfg->num_envs + 1; env++) {
    std::vector<uint32_t> lds(words, 0xC3C3C3C3u + (uint32_t)env);
    AuditWaveHost w;
    if (map) audit_body<AuditWaveHost, 1>(w, lds.data(), env, *cfg, *tb, *st, mask, flags, detail);
    else audit_body<AuditWaveHost, 0>(w, lds.data(), env, *cfg, *tb, *st, mask, flags, detail);
  }
  return 0;
}

int hostsim_audit_in_wave(const Config* cfg) { return audit_in_wave(*cfg) ? 1 : 0; }
int hostsim_audit_lds_bytes(const Config* cfg) { return (int)(audit_lds_words(*cfg) * 4); }

}  // extern "C"
