/* libcrafter_hip.so -- nearby queries: an extension of the C ABI of crafter_hip.h, in a header of its own (as
 * crafter_hip_navigate.h: crafter_hip.h's set of prototypes is pinned, an entry point added under the same ABI revision is
 * declared beside it and listed in the Python binding's lib.EXTENSIONS).  C99, includes crafter_hip.h.
 */
#ifndef CRAFTER_HIP_NEARBY_H_
#define CRAFTER_HIP_NEARBY_H_

#include "crafter_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CRAFTER_NEARBY_CLIP 0       /* flags: the window is the square clipped to the world (the default) */
#define CRAFTER_NEARBY_NUMPY 1      /* flags: the window is what the reference's numpy slices select */
#define CRAFTER_NEARBY_MAX_ENTS 32  /* rows of the entity list per env */
#define CRAFTER_NEARBY_ROW 6        /* int16 per row: class, dx, dy, health, facing code, aux */
#define CRAFTER_NEARBY_MAX_SIDE 512 /* the entity list's sort key holds |dx| <= 511: W and H at most this with k > 0 */

/* Nearby queries: for masked envs (NULL: all; rows with a zero mask byte are left untouched), what World.nearby(player.pos,
 * distance) and World.count(material) say about the world (engine.py:95-110), as counts per class, and the k nearest objects.
 * Env e as it stands on `stream`, p the player's cell (slot 1 of the slot table), d = distance:
 *   window            flags == CRAFTER_NEARBY_CLIP: the cells inside the world with |x - p.x| <= d and |y - p.y| <= d; the whole
 *                     world for d < 0.
 *                     flags == CRAFTER_NEARBY_NUMPY: exactly the cells of _mat_map[x - d: x + d + 1, y - d: y + d + 1].  Per axis of
 *                     length L: start = p - d; if start < 0, start += L; if it is still negative, start = 0; stop = min(p + d + 1, L);
 *                     the axis is empty if start >= stop.  (One or two cells from the west or north border the window is EMPTY: the
 *                     reference cannot craft there.  For d >= L the clipped start brings the whole axis back.)  d < 0 is refused.
 *   class ids         those of crafter_symbolic plane 0: 0 none, a material's id (1 + position in the rules' materials), n_materials
 *                     + type (CRAFTER_T_PLAYER .. CRAFTER_T_PLANT) for an object.  C = 1 + n_materials + 6 columns.
 *   counts[e][0]      the number of cells in the window
 *   counts[e][m]      1 <= m <= n_materials: the window cells whose material is m, whatever stands on them (World.count for the
 *                     whole world; the non-zero columns are World.nearby(...)[0])
 *   counts[e][n_materials + t]   the live objects of type t in the window, the player included (World.nearby(...)[1] by class)
 *   n[e]              the live objects in the window whose class is in the 32-bit set `classes` (bit c = class c).  May exceed k.
 *   ents[e][j]        j < min(n[e], k): the j-th of those objects in ascending dx^2 + dy^2, then ascending dx, then ascending dy
 *                     (dx, dy = its cell - p; a cell holds one object, so the order is total and independent of slot order), as
 *                     (class id, dx, dy, health, facing code, aux): the facing code is crafter_symbolic plane 1's variant (arrow
 *                     1 .. 4 = left, right, up, down; plant 1 if ripe; the player 1 .. 4 or 5 asleep; else 0), the player's health
 *                     is its inventory's, aux is saturated to int16.  Rows j >= min(n[e], k) are written as zeros.
 * A row that was never reset (and one whose player record lies outside the world) gives all zeros.
 *   counts: int32 [num_envs][C];  ents: int16 [num_envs][k][CRAFTER_NEARBY_ROW];  n: int32 [num_envs].  k == 0 skips the list:
 *   ents and n may then be NULL and are not written.
 * mask, counts, ents and n are device pointers.  Read-only: no draw from the env's RNG, no byte of state changes, nothing of the
 * world pool is looked at; reads live rows only: no wait for the world pool.  Worlds of at most 64 x 64 cells are served by one
 * wavefront per env, larger ones by one workgroup per env; no global atomics, and every integer is the same whatever order the
 * lanes reduce in.  Only enqueues work; returns 0, or non-zero with crafter_last_error: k outside 0 .. CRAFTER_NEARBY_MAX_ENTS,
 * flags other than the two above, a `classes` bit outside the object classes, CRAFTER_NEARBY_NUMPY with distance < 0, a NULL
 * counts, a NULL ents or n with k > 0, rules with more than 31 classes, k > 0 on a world with a side above
 * CRAFTER_NEARBY_MAX_SIDE or a slot table beyond the kernel's 64 KiB of LDS (about 16000 slots).
 * Additive under ABI revision 7: a binding looks it up by name. */
int crafter_nearby(crafter_handle* h, const uint8_t* mask, int32_t distance, int32_t flags, uint32_t classes, int32_t k,
                   int32_t* counts, int16_t* ents, int32_t* n, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CRAFTER_HIP_NEARBY_H_ */
