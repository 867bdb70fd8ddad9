/* libcrafter_hip.so -- edits of envs in place: an extension of the C ABI of crafter_hip.h, in a header of its own (as
 * crafter_hip_fingerprint.h and crafter_hip_navigate.h: crafter_hip.h's set of prototypes is pinned, an entry point added under
 * the same ABI revision is declared beside it and listed in the Python binding's lib.EXTENSIONS).  C99, includes crafter_hip.h.
 */
#ifndef CRAFTER_HIP_EDIT_H_
#define CRAFTER_HIP_EDIT_H_

#include "crafter_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sticky status bit of an env (crafter_env_rec.status): an edit tape held an op the device refused or repaired (the cases below).
 * The next free bit behind CRAFTER_ST_BAD_WORLD (128, crafter_hip.h). */
#define CRAFTER_ST_BAD_EDIT 256u

/* One op is eight int32 words: word 0 the kind, words 1 .. 7 its arguments in the order given here; words an op does not name
 * are ignored.  (x, y) is a cell of the world map, indexed as the reference's world[x, y]. */
#define CRAFTER_EDIT_WORDS 8
enum {
  CRAFTER_EDIT_NOP = 0,        /* --                                                                                       */
  CRAFTER_EDIT_SET_CELL = 1,   /* x y material          world[x, y] = material                        engine.py:82-86      */
  CRAFTER_EDIT_ADD = 2,        /* type x y health fx fy aux   world.add(cls(world, (x, y))), then the fields   engine.py:50-57 */
  CRAFTER_EDIT_REMOVE = 3,     /* x y                   world.remove(world[x, y][1])                  engine.py:59-65      */
  CRAFTER_EDIT_MOVE = 4,       /* x y x2 y2             world.move(world[x, y][1], (x2, y2))          engine.py:67-80      */
  CRAFTER_EDIT_SET_OBJECT = 5, /* x y which health fx fy aux   obj.health / obj.facing / obj.cooldown | reload | grown = ... */
  CRAFTER_EDIT_SET_ITEM = 6,   /* item value            player.inventory[item] = value                                     */
  CRAFTER_EDIT_SET_PLAYER = 7, /* field value           player.sleeping / _hunger / _thirst / _fatigue / _recover = ...    */
  CRAFTER_EDIT_SET_CLOCK = 8,  /* step                  env._step = step; env._update_time()          env.py:135-139       */
  CRAFTER_EDIT_KINDS = 9
};
/* SET_OBJECT's `which`: the fields the op assigns */
enum { CRAFTER_EDIT_HEALTH = 1, CRAFTER_EDIT_FACING = 2, CRAFTER_EDIT_AUX = 4 };
/* SET_PLAYER's `field`, in the units crafter_env_rec keeps (twice the reference's half-step counters) */
enum { CRAFTER_EDIT_SLEEPING = 0, CRAFTER_EDIT_HUNGER2 = 1, CRAFTER_EDIT_THIRST2 = 2, CRAFTER_EDIT_FATIGUE2 = 3,
       CRAFTER_EDIT_RECOVER2 = 4, CRAFTER_EDIT_FIELDS = 5 };

/* Edits n envs in place, between two steps: for each i < n the ops ops[i][0 .. ops_per_env) are applied to env idx[i], in order.
 * Each op means exactly what the reference statement beside its kind means when executed between two Env.step calls:
 *   SET_CELL    the map only: an object on the cell stays.  The per-chunk grass / path census follows.
 *   ADD         type CRAFTER_T_COW .. CRAFTER_T_PLANT on a cell free of objects (the material is not looked at); the object is
 *               appended to the slot table, its chunk's key to the chunk order at first touch, the creature census follows.
 *               health, facing and aux (zombie cooldown / skeleton reload / plant grown) as a record of crafter_reset_worlds'
 *               bank: health is kept in the record's signed byte, only an arrow keeps a facing (the others' is (0, 0)).
 *   REMOVE      the object on the cell, never the player.
 *   MOVE        the object on (x, y), the player too, to (x2, y2): inside the map and free of objects; the material is not
 *               looked at, as in the reference.  A new chunk's key is appended, the creature census follows.
 *               (x2, y2) == (x, y) changes nothing.
 *   SET_OBJECT  the fields `which` names of the object on the cell.  The player has a facing only (its health is an item).
 *               A facing given to a class that keeps none is ignored.
 *   SET_ITEM    item = index into the rules' items; the value is clamped to 0 .. the item's maximum.  Player._last_health and
 *               Env._last_health are left alone: the next step's reward sees a health change as the reference's does.
 *   SET_PLAYER  sleeping 0 / 1, hunger2 0 .. 50, thirst2 0 .. 40, fatigue2 -20 .. 60, recover2 -30 .. 50 (what the rules can
 *               leave in them, objects.py:133-167).
 *   SET_CLOCK   0 <= step < the daylight table's length, and < Config.length where that is not 0; crafter_render,
 *               crafter_symbolic and the next step see that step's daylight.
 * An edit draws nothing from the env's RNG, does not redraw obs (crafter_render does, with the noise a night frame draws), does
 * not touch reward, done, info['semantic'], the terminal row, the episode counters, the seed lane or the world pool's entries,
 * neither reads nor writes the row of an env idx does not name, and does not wait for the world pool.  An edited episode ends
 * and auto-resets like any other.
 *
 * The tape comes from a caller and is never trusted.  These ops are skipped, or repaired where that is said, and set the sticky
 * CRAFTER_ST_BAD_EDIT in the env's status; the other ops of the tape are applied and the row stays consistent:
 *   - a kind outside 0 .. CRAFTER_EDIT_KINDS - 1;
 *   - SET_CELL, ADD, REMOVE, MOVE (either cell), SET_OBJECT: a cell outside the map;
 *   - SET_CELL: a material id outside 1 .. n_materials;
 *   - ADD: a type that is none, the player or no class; a cell that holds an object; an arrow whose facing is no unit axis
 *     vector (repaired to (0, 1): the arrow is added);
 *   - REMOVE, SET_OBJECT: no object on the cell;  REMOVE: the object is the player;
 *   - MOVE: no object on (x, y); (x2, y2) holds another object;
 *   - SET_OBJECT: `which` with a bit above CRAFTER_EDIT_AUX (repaired: the known bits are applied); health or aux on the
 *     player (repaired: a facing in the same op is applied); a facing for the player or an arrow that is no unit axis vector
 *     (repaired: the op's other fields are applied);
 *   - SET_ITEM: an item outside the rules' items; a value outside 0 .. the item's maximum (repaired: clamped);
 *   - SET_PLAYER: a field outside 0 .. CRAFTER_EDIT_FIELDS - 1; a value outside the field's range;
 *   - SET_CLOCK: a step outside the range above.
 * An ADD into a full slot table sets CRAFTER_ST_OBJ_OVERFLOW, as World.add does everywhere.
 *
 *   idx:  int32 [n], as for crafter_step_envs: checked on the device before any env is edited; a list with an entry outside
 *         0 .. num_envs - 1 or naming an env twice refuses the whole call -- no row changes -- and sets CRAFTER_ST_BAD_COPY in
 *         the status of every named row that exists (row 0 if none does)
 *   ops:  int32 [n][ops_per_env][CRAFTER_EDIT_WORDS], 16-byte aligned, padded with NOP
 * idx and ops are device pointers.  Only enqueues work; n == 0 enqueues nothing.  Returns 0, or non-zero with
 * crafter_last_error: n outside 0 .. num_envs, a NULL idx or ops, ops_per_env < 1, ops not 16-byte aligned.  Additive under ABI
 * revision 7: a binding looks it up by name. */
int crafter_edit_envs(crafter_handle* h, const int32_t* idx, int32_t n, const int32_t* ops, int32_t ops_per_env, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CRAFTER_HIP_EDIT_H_ */
