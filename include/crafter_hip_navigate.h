/* libcrafter_hip.so -- navigation queries: an extension of the C ABI of crafter_hip.h, in a header of its own (as
 * crafter_hip_fingerprint.h: crafter_hip.h's set of prototypes is pinned, an entry point added under the same ABI revision is
 * declared beside it and listed in the Python binding's lib.EXTENSIONS).  C99, includes crafter_hip.h.
 */
#ifndef CRAFTER_HIP_NAVIGATE_H_
#define CRAFTER_HIP_NAVIGATE_H_

#include "crafter_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CRAFTER_NAV_MAX_TARGETS 16   /* target sets per call */

/* Navigation queries: for masked envs (NULL: all; rows with a zero mask byte are left untouched) and each of k target sets,
 * how many steps on foot the nearest target is from the player and which move comes first (no reference counterpart as a
 * call; every value follows Object.is_free objects.py:44-47, Object.move 36-42 and SemanticView engine.py:251-264).
 * Env e as it stands on `stream`:
 *   class of a cell   the id info['semantic'] / crafter_symbolic plane 0 gives it: n_materials + type (CRAFTER_T_PLAYER ..
 *                     CRAFTER_T_PLANT) of the object standing on it, else its material id (1 + position in the rules' materials);
 *                     the classes are 0 (none) .. n_materials + 6
 *   target            a 32-bit set of class ids: bit c set = class c counts
 *   passable          a 32-bit set of material ids (the reference's `walkable`, crafter_rules.walkable_mask, is what a plain
 *                     object walks on; the player's own set adds lava)
 *   T_k               the cells inside the world whose class is in targets[k], except the player's own cell
 *   P                 the cells inside the world whose material is in `passable` and that hold no object, plus the player's cell
 *   dist(c)           0 for c in T_k; for c in P \ T_k, 1 + the minimum of dist(n) over the four neighbours n of c that lie in
 *                     T_k or P; infinite where no such chain exists
 *   dist[e][k]        dist(the player's cell), or -1 if infinite.  Always >= 1 or -1: the number of move actions after which the
 *                     player faces the target -- or stands on it, if the target is passable and free -- provided nothing else moves
 *   first[e][k]       the index in the uploaded rules' action list of the move action of the first direction, in the order
 *                     left (-1, 0), right (+1, 0), up (0, -1), down (0, +1), whose neighbour n is inside the world, in T_k or P
 *                     and has dist(n) = dist - 1; -1 where dist is -1 (or the rules hold no such action)
 *   facing[e][k]      1 iff the cell pos + facing is inside the world and in T_k ("`do` now"), else 0
 * The query ignores sleeping, damage and what creatures will do next.  After a crafter_step that auto-reset an env the row
 * describes the new episode's first state, after a rollout the state behind its last step (as crafter_symbolic).
 *   targets:  HOST array of k class sets, read before the call returns (they travel as kernel arguments)
 *   dist, first:  int32 [num_envs][k];  facing: uint8 [num_envs][k] or NULL
 * mask, dist, first and facing are device pointers.  Read-only: no draw from the env's RNG, no byte of state changes, nothing of
 * the world pool is looked at; reads live rows only: no wait for the world pool.  Worlds of at most 64 x 64 cells are searched
 * by one wavefront per env with the boards in registers, larger ones by one workgroup per env with the boards in LDS
 * (areas whose five boards exceed 64 KiB of LDS -- beyond about 100000 cells -- are refused).  Only enqueues work; returns 0, or
 * non-zero with crafter_last_error: k outside 1 .. CRAFTER_NAV_MAX_TARGETS, a NULL targets, a target of 0, with bit 0 set or
 * with a bit at or above the class count, `passable` with bit 0 set or a bit above the materials, a NULL dist or first, rules
 * with more than 31 classes.  Additive under ABI revision 7: a binding looks it up by name. */
int crafter_navigate(crafter_handle* h, const uint8_t* mask, const uint32_t* targets, int32_t k, uint32_t passable,
                     int32_t* dist, int32_t* first, uint8_t* facing, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CRAFTER_HIP_NAVIGATE_H_ */
