// TEST INFRASTRUCTURE -- crafter_fingerprint's body (csrc/fingerprint.hpp) on the CPU through WaveHost (see wave_host.hpp).
#include <string.h>

#include "wave_host.hpp"
#include "../../crafter_amd/csrc/fingerprint.hpp"

using namespace crafter;

// WaveHost plus the primitives fingerprint.hpp adds to the wave policy (wave_gfx950.hpp sum64, lane_gather4).
struct FingerprintWaveHost : WaveHost {
  // one host thread plays the 64 lanes one after the other into the same accumulator: what a "lane" holds at the end is the
  // wave's sum already
  static uint64_t sum64(uint64_t v) { return v; }
  // (predicated where the device clamps: the record at n - 1 is read by the lanes it belongs to only)
  template <int R0, int K, class T>
  void lane_gather4(int base, int n, const T* rec) {
    static_assert(sizeof(T) == 16, "16-byte records");
    for (int k = 0; k < K; k++)
      for (int lane = 0; lane < 64; lane++) {
        const int i = base + 64 * k + lane;
        uint32_t words[4] = {0u, 0u, 0u, 0u};
        if (i < n) memcpy(words, rec + i, 16);
        for (int j = 0; j < 4; j++) lv[R0 + 4 * k + j][lane] = words[j];
      }
  }
};

extern "C" {

// cfg / tb / st: a HostSimEnv's.  key: [N] or null; part_hash: [N][7] or null.
int hostsim_fingerprint(const Config* cfg, const TablePtrs* tb, const StatePtrs* st, const uint8_t* mask, uint32_t parts, uint64_t* key,
                        uint64_t* part_hash) {
  if ((!key && !part_hash) || (parts & ~kFpAll) || (key && !parts)) return 1;   // what crafter_fingerprint refuses
  // one env beyond the batch, as the last workgroup's spare waves: must return without touching anything
  for (int env = 0; env < cfg->num_envs + 1; env++) {
    FingerprintWaveHost w;
    fingerprint_body<FingerprintWaveHost>(w, env, *cfg, *tb, *st, mask, parts, key, part_hash);
  }
  return 0;
}

}  // extern "C"
