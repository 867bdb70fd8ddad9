/* libcrafter_hip.so -- state fingerprints: an extension of the C ABI of crafter_hip.h, in a header of its own.
 *
 * crafter_hip.h is the core boundary, and its set of prototypes is pinned (tests/test_host_logic.py holds crafter_amd/lib.py's
 * signature table against it name by name).  An entry point added under the same ABI revision that a binding looks up by name
 * is declared here instead; the Python binding lists it in lib.EXTENSIONS.  C99, includes crafter_hip.h; the part constants
 * CRAFTER_FP_* are crafter_hip_types.h's.
 */
#ifndef CRAFTER_HIP_FINGERPRINT_H_
#define CRAFTER_HIP_FINGERPRINT_H_

#include "crafter_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* State fingerprints: 64-bit keys that say whether two envs are in the same state (no reference counterpart as a call), for
 * masked envs (NULL: all; rows with a zero mask byte are left untouched).  What is hashed is the canonical state -- what
 * copy.deepcopy of the reference's Env would carry, in one fixed form -- never the raw buffers: free slot-table records behind
 * nobj, the T_NONE holes of a table, crafter_obj.pad, the player's crafter_obj.health byte, objmap, census, chunk_seen, status,
 * dhealth / new_unlocked / dead / done / needs_reset, the ep_* totals, env_last_health and unlocked (both derived), the world
 * pool and obs / reward / done do NOT enter.  NOT cryptographic: a mixing hash for transposition tables, archives and
 * duplicate checks.
 *   mix64(z):  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^ z >> 31   (as `pick`)
 *   G = 0x9E3779B97F4A7C15;  all arithmetic mod 2^64;  S_p = mix64(p + 1) is the salt of part p
 *   a part is n 64-bit units u_0 .. u_{n-1}:  H_p = mix64(S_p + n + sum_i mix64((u_i ^ S_p) + (i + 1) * G))
 *   K(parts) = mix64((uint64)parts * G + sum_{p in parts} H_p)
 * The parts, bit p of `parts` = CRAFTER_FP_* (crafter_hip_types.h):
 *   p  name     units
 *   0  MAP      the env's mat row (W * H bytes), 8 bytes per unit, little-endian, the last unit zero-padded: n = ceil(W * H / 8)
 *   1  OBJECTS  the live objects in slot order -- slots 1 .. min(nobj, max_objects) - 1 with type != CRAFTER_T_NONE; the object
 *               of rank k among them gives unit 2k = type | (health & 0xFF) << 8 | (fx & 0xFF) << 16 | (fy & 0xFF) << 24 |
 *               x << 32 | y << 48, where a PLAYER record's health is inv[item_health], and unit 2k + 1 = (uint32)aux.  Rank,
 *               not slot number: holes do not count
 *   2  PLAYER   one unit per value, each (uint32) zero-extended: inv[0 .. n_items), ach[0 .. n_achievements), sleeping != 0,
 *               hunger2, thirst2, fatigue2, recover2, player_last_health
 *   3  CLOCK    (uint32)step
 *   4  RNG      mt[2i] | mt[2i + 1] << 32 for i < 312, then (uint32)mt_pos
 *   5  CHUNKS   chunk_order[0 .. min(nchunks_seen, nch)), one unit each
 *   6  IDENT    seed_lane, then (uint32)episode
 * CRAFTER_FP_VISIBLE = MAP | OBJECTS | PLAYER; CRAFTER_FP_DYNAMICS = every part but IDENT: two envs with equal DYNAMICS keys are
 * meant to produce identical outputs under any common action sequence until the episode ends; CRAFTER_FP_ALL.
 *   key:        uint64 [num_envs] or NULL: K(parts)
 *   part_hash:  uint64 [num_envs][CRAFTER_FP_PARTS] or NULL: H_0 .. H_6, whatever `parts` says
 * All pointers are device pointers.  Read-only: no draw from the env's RNG, no byte of state changes.  Reads live rows only: no
 * wait for the world pool.  Only enqueues work; returns 0, or non-zero with crafter_last_error: both outputs NULL, a bit of
 * `parts` above CRAFTER_FP_IDENT, or parts == 0 with key != NULL.  Additive under ABI revision 7: a binding looks it up by name. */
int crafter_fingerprint(crafter_handle* h, const uint8_t* mask, uint32_t parts, uint64_t* key, uint64_t* part_hash, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CRAFTER_HIP_FINGERPRINT_H_ */
