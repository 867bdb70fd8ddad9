/* libcrafter_hip.so -- C ABI of the MI355X-native batched Crafter hot path.
 *
 * The reference (danijar/crafter) is pure Python and has no FFI; the boundary it offers for this
 * path is the Python surface of crafter/env.py:
 *     Env.__init__ (env.py:27-56)  Env.reset (env.py:70-81)  Env.step (env.py:83-118)
 *     Env.render (env.py:120-130)  info['semantic'] (engine.py:251-264)
 * Each entry point below names the reference interface it replaces.  The host side that binds
 * them (ctypes) and mirrors crafter.Env is crafter_amd/{lib,batched,env}.py; INTEGRATION.md shows
 * the stub a reference maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types cross this boundary;
 *   - "device pointer" = address in GPU memory owned by the CALLER (e.g. torch tensor data_ptr);
 *     the library never frees or reallocates caller memory; its own scratch lives in the handle;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every call only
 *     ENQUEUES work on that stream, there are no hidden synchronisations after crafter_create /
 *     crafter_upload_tables;
 *   - return 0 on success, non-zero on error with text in crafter_last_error(); nothing throws;
 *   - calls on one handle must be serialised by the caller.
 *
 * Struct layouts (crafter_config, crafter_rules, crafter_state_ptrs, crafter_obj, crafter_env_rec) are plain C99
 * in crafter_hip_types.h, included below: this header is self-contained for a C / Rust / Go / Java binding
 * (tests/c/boundary_test.c drives the whole path from C with nothing else).  That file is the only statement of the
 * layouts: the library's kernels are compiled against it (crafter_amd/csrc/types.hpp merely aliases its structs).
 * crafter_amd/abi.py is the ctypes mirror, checked against it offset by offset in the test suite, and
 * crafter_struct_sizes lets any binding verify its own.
 */
#ifndef CRAFTER_HIP_H_
#define CRAFTER_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crafter_handle crafter_handle;
#include "crafter_hip_types.h"

/* Host-side tables handed to crafter_upload_tables (all HOST pointers, copied by the library).
 * They carry everything the reference evaluates with numpy / Pillow / its yaml at run time:
 * data.yaml rules (constants.py:6-8), the resized textures (engine.py:131-142), daylight(step)
 * (env.py:135-139) and the night vignette (engine.py:213-218). */
typedef struct crafter_host_tables {
  const crafter_rules* rules;
  const uint8_t* atlas;      size_t atlas_bytes;   /* RGBA texels, [x][y] per texture          */
  const int32_t* tex_tile;   int32_t n_tex_tile;   /* byte offsets, CRAFTER_TEX_* slots         */
  const int32_t* tex_icon;   int32_t n_tex_icon;   /* per item                                 */
  const int32_t* tex_digit;  int32_t n_tex_digit;  /* '1'..'9' at [1..9], 'unknown' at [10]    */
  const uint8_t* tex_alpha;  int32_t n_tex_alpha;  /* 1 = source PNG had an alpha channel      */
  const int32_t* item_pos;   int32_t n_item_pos;   /* [items][4] icon x,y / digit x,y          */
  const double* daylight;    int32_t n_daylight;
  const double* vignette;    int32_t n_vignette;   /* local_w * local_h                        */
  const float* unit255;      int32_t n_unit255;    /* 256                                      */
} crafter_host_tables;

/* sizeof(Obj, EnvRec, Rules, Config, StatePtrs, TablePtrs) as compiled, for binding self-checks. */
void crafter_struct_sizes(int32_t out[6]);

/* ABI revision of this header.  Revision 7 includes the additive entry points crafter_copy_envs, crafter_save_envs and
 * crafter_load_envs (and the status bit CRAFTER_ST_BAD_COPY): a binding looks them up by name. */
int32_t crafter_abi_version(void);

/* Replaces Env.__init__ (env.py:27-56) for a batch of cfg->num_envs environments. */
int crafter_create(const crafter_config* cfg, crafter_handle** out);
void crafter_destroy(crafter_handle* h);

/* Replaces the import-time loading of data.yaml / assets and the numpy evaluation of daylight and
 * vignette (constants.py:6-8, engine.py:122-129,213-218, env.py:135-139).  Synchronous copy. */
int crafter_upload_tables(crafter_handle* h, const crafter_host_tables* t);

/* Env(length=None) (env.py:29: no time limit; env.py:135-139 _update_time is evaluated by the host into the daylight table,
 * one value per step of an episode): replaces the handle's daylight table by a longer one -- daylight[0 .. n), n greater
 * than the current size, the first entries equal to the current table's -- so that an episode can run past the table it
 * started with.  A step beyond the table is clamped to its last entry and sets CRAFTER_ST_STEP_OVERFLOW.  Synchronous copy;
 * launches already enqueued keep the table they were launched with.  Handles created with fewer than 1024 daylight steps
 * cannot grow. */
int crafter_extend_daylight(crafter_handle* h, const double* daylight, int32_t n);

/* Registers the caller-owned device buffers holding the world state (sizes: crafter_amd/state.py). */
int crafter_bind_state(crafter_handle* h, const crafter_state_ptrs* state);

/* Bytes of LDS one environment's workgroup uses (diagnostics / occupancy planning). */
int32_t crafter_lds_bytes(const crafter_handle* h);

/* 1: the world maps are staged in LDS and the cell -> slot map (the reference's World._obj_map,
 * engine.py:32) is derived state, rebuilt from the slot table (World._objects, engine.py:33) at every
 * stage-in: crafter_state_ptrs.objmap is then never read or written.  0: large world, both maps live
 * in HBM and objmap is kept current. */
int32_t crafter_slot_map_derived(const crafter_handle* h);

/* Environment variables.  The library reads four, all DISPATCH OVERRIDES between kernels it ships (tests drive each kernel at
 * every batch size with them; none is needed in normal use), at crafter_create:
 *   CRAFTER_ORDER=0|1       dispatch order of the step launch (slow envs first) never / always   (default: batches > 1280 envs)
 *   CRAFTER_SPLIT=0|1       the default instance as one fused step kernel / as rules kernel + frame kernel (default: the pair
 *                           only when no frame is drawn)
 *   CRAFTER_STEP_WIDE=0|1   the default instance with 512 threads per env never / always          (default: batches <= 512 envs)
 *   CRAFTER_STEP_EARLY=0|1  the default instance as the kernel whose day frames begin before the rules end, never / always
 *                                                                                                  (default: batches >= 2048 envs)
 * Experiment knobs and timing probes exist only in builds with -DCRAFTER_PROBES (Diagnostics). */

/* Which instance of the step kernel crafter_step launches for this handle (diagnostics): bit 2 = maps staged in
 * LDS, bit 1 = the default geometry of crafter.Env() (env.py:27-46) compiled in, bit 0 = the uploaded rules equal
 * the compiled-in data.yaml (call after crafter_upload_tables).  7 = the fast path everybody should be on.  Bit 3 (9): a
 * world too large for LDS (maps and slot table stay in global memory) seen through the default view with the default rules,
 * both compiled in -- crafter_step_kernel<0, 2, 1>, BASELINE configs[3]. */
int32_t crafter_step_instance(const crafter_handle* h);

/* Replaces Env.reset (env.py:70-81) for every env whose mask byte is non-zero (mask == NULL: all).
 * mask: device uint8[num_envs].  obs: device uint8[num_envs][size_h][size_w][3] or NULL. */
int crafter_reset(crafter_handle* h, const uint8_t* mask, uint8_t* obs, void* stream);

/* Authored worlds: Env.reset (env.py:70-81) with worldgen.generate_world(world, player) replaced by "write this map, add these
 * objects" -- the env then stands in a world the CALLER designed (additive under revision 7: a binding looks the entry point
 * up by name).  For every env whose mask byte is non-zero, with j = world_id[env] (world_id == NULL: env % n_worlds):
 *     world material map[:] = bank_mat[j]                               [W][H], index x * H + y
 *     for r in bank_objs[j][0 .. bank_nobj[j]), in order:
 *         r.type == CRAFTER_T_PLAYER (allowed as record 0 only):
 *             if (r.x, r.y) is not the centre: World.move(player, (r.x, r.y));  player.facing = (r.fx, r.fy)
 *         else: World.add(Cow | Zombie | Skeleton | Arrow | Plant at (r.x, r.y)) with health = r.health, r.aux as the zombie's
 *             cooldown / the skeleton's reload / the plant's grown, and for an arrow facing = (r.fx, r.fy)
 *     player.inventory = bank_inv[j]                                    if given; else the rules' initial inventory
 * Everything before and after is Env.reset unchanged: the episode counter advances by one, World.reset, RandomState(world
 * seed) seeded exactly as crafter_reset seeds it (a level table in force included), the player added at the centre first (slot
 * 1; its chunk is the first chunk key), step 0, hunger / thirst / fatigue / recover and the achievements cleared, the first
 * frame drawn.  The authored function draws nothing: the episode's stream starts at the first word of RandomState(world seed).
 * Slots are 2, 3, ... in record order, chunk keys are inserted in the order the calls above touch them, and every derived
 * table of the row (cell -> slot map, census, nobj) is what those calls leave.  An authored world lasts ONE episode: the next
 * one is the ordinary generated episode k + 1 of the env's seed.
 *
 * The bank is checked on the device, record by record; nothing in it can make a kernel read or write outside a table.  Each of
 * the following sets the sticky CRAFTER_ST_BAD_WORLD in the env's record, and the reset still completes into a consistent row:
 *   - a material byte outside 1 .. n_materials is written as rules.mat_grass;
 *   - a record is skipped if its type is none of the six classes, if its cell lies outside the world or is already
 *     occupied, or if it is a PLAYER record other than record 0;
 *   - a facing (player, arrow) that is no unit axis vector is written as (0, 1).  The other classes keep no facing: their
 *     fx / fy are ignored and stored as (0, 0), as World.add's other callers store them.
 * A world id outside 0 .. n_worlds - 1 sets the bit and leaves the row (and its pool entries) untouched.  Records beyond the
 * batch's slot table set CRAFTER_ST_OBJ_OVERFLOW, as every World.add does.  A PLAYER record's health and aux are ignored
 * (the player's health is the inventory's).
 *
 * All pointers are device pointers.  mask: uint8[num_envs] or NULL (all), as for crafter_reset; rows with a zero byte are
 * neither read nor written.  world_id: int32[num_envs] or NULL.  bank_mat: uint8[n_worlds][W * H].  bank_objs:
 * crafter_obj[n_worlds][bank_max_objects], 16-byte aligned.  bank_nobj: int32[n_worlds], taken as clamped to
 * 0 .. bank_max_objects.  bank_inv: int32[n_worlds][rules.n_items] or NULL, each value taken as clamped to 0 .. item_max.
 * obs as for crafter_reset.  Host-side errors: a NULL bank_mat / bank_objs / bank_nobj, a misaligned bank_objs,
 * n_worlds < 1, bank_max_objects < 0.  The call only enqueues; the bank must stay alive and unchanged until the work has run.
 * It is ordered behind the world pool exactly as crafter_reset is, and afterwards each env does to its pool entries exactly
 * what crafter_reset does (the next episode's world is generated into its entry, the one after is requested).
 * A bank drawn from by the AUTOMATIC reset inside crafter_step is deliberately not offered. */
#define CRAFTER_ST_BAD_WORLD 128   /* sticky status bit, beside CRAFTER_ST_* of crafter_hip_types.h */
int crafter_reset_worlds(crafter_handle* h, const uint8_t* mask, const int32_t* world_id, const uint8_t* bank_mat,
                         const crafter_obj* bank_objs, const int32_t* bank_nobj, const int32_t* bank_inv, int32_t n_worlds,
                         int32_t bank_max_objects, uint8_t* obs, void* stream);

/* Replaces Env.step (env.py:83-118) for all envs.
 * actions: device int32[num_envs]; obs as above; reward: device float[num_envs];
 * done: device uint8[num_envs].  With cfg->auto_reset, envs that finished are regenerated
 * (Env.reset) before the call's work completes and their obs is the new episode's first frame.
 * info[...] of the reference is read from the bound state buffers (EnvRec.inv/ach/..., semantic). */
int crafter_step(crafter_handle* h, const int32_t* actions, uint8_t* obs, float* reward, uint8_t* done,
                 void* stream);
/* Copies of whole environments (the reference's copy.deepcopy / pickle of a crafter.Env carries everything below).  An env
 * row is: mat, objs (the whole slot table), mt, rec (step / episode counters, seed lane, sticky status...), chunk_order,
 * chunk_seen, census, terminal, semantic (if kept), objmap (only where crafter_slot_map_derived() == 0) and the row of the
 * caller's obs / reward / done buffers (NULL: not copied).  DESIGN.md 3 lists what is state, derived and scratch.
 * Indices are device int32 arrays.  They are checked on the device before anything is copied: an index out of range, a
 * destination named twice, or (crafter_copy_envs) a destination that is also a source refuses the WHOLE call -- no row
 * changes -- and sets CRAFTER_ST_BAD_COPY in the status of the bound-state rows it names (row 0 if none exists).
 *
 * crafter_copy_envs: row dst[i] of the bound state becomes an exact copy of row src[i], i < n, as it stands after every call
 *   enqueued before.  With the world pool running the source's two pooled worlds go along, so that the copy's later episodes
 *   come from the pool too.  Before the copy the pool is brought to rest: the requests collected so far are launched as a batch
 *   and the stream waits (on the device) for every batch launched; the cost is measured in DESIGN.md 9.
 * A store: a crafter_state_ptrs with the pool and queue pointers NULL (objmap only where the map is state, semantic only if
 *   kept), `store_rows` rows and a slot table of `store_max_objects` entries, plus obs / reward / done rows of the batch's
 *   layout.  Geometry, view, size, rules and length are those of the handle; the caller keeps them equal.
 * crafter_save_envs: store row i <- bound row idx[i], i < n <= store_rows; store_max_objects >= the handle's.  Reads live rows
 *   only: no wait for the pool.
 * crafter_load_envs: bound row idx[i] <- store row rows[i] (rows NULL: i); store_max_objects <= the handle's (a narrower
 *   table is zero-padded).  The destination's pool entries are emptied: it regenerates its next world inline once (same
 *   generator, same (seed, episode): unobservable) and the pool takes over again.  Brings the pool to rest first, as above. */
int crafter_copy_envs(crafter_handle* h, const int32_t* src, const int32_t* dst, int32_t n, uint8_t* obs, float* reward, uint8_t* done,
                      void* stream);
int crafter_save_envs(crafter_handle* h, const int32_t* idx, int32_t n, const uint8_t* obs, const float* reward, const uint8_t* done,
                      const crafter_state_ptrs* store, int32_t store_rows, int32_t store_max_objects, uint8_t* store_obs,
                      float* store_reward, uint8_t* store_done, void* stream);
int crafter_load_envs(crafter_handle* h, const crafter_state_ptrs* store, int32_t store_rows, int32_t store_max_objects,
                      const uint8_t* store_obs, const float* store_reward, const uint8_t* store_done, const int32_t* rows,
                      const int32_t* idx, int32_t n, uint8_t* obs, float* reward, uint8_t* done, void* stream);

/* Streams: a handle's calls are ordered by the stream they are issued on.  Changing the stream between two calls
 * (crafter_reset on one, crafter_step on another) is allowed: the library makes the new stream wait for the work the
 * handle still has in flight on the previous one and for the world pool's side streams, then carries on there.  Two
 * streams ALTERNATING every call therefore serialise; use one stream per handle.
 * With auto-reset and the world pool running, an env that finishes and finds no world in the pool (all but never one) is
 * regenerated by a second kernel behind the step launch, on the same stream: every output of the call is complete in
 * stream order. */

/* `steps` consecutive calls of crafter_step in one (Env.step, env.py:83-118, in a loop such as run_random.py:36-44) for
 * policies that choose their actions without looking at the observations (random, scripted, action repeat):
 * actions: device int32[steps][num_envs]; obs: device uint8[steps][num_envs][size_h][size_w][3] or NULL;
 * reward: device float[steps][num_envs]; done: device uint8[steps][num_envs].  Bit-identical to the loop; faster because
 * an env starts its step t + 1 without waiting for every other env's step t.  One launch covers the steps up to the world
 * pool's next generation batch, or 16 steps when the pool is off (so that an env that finished waits at most that long for the
 * launch boundary its inline regeneration happens at). */
int crafter_step_n(crafter_handle* h, int32_t steps, const int32_t* actions, uint8_t* obs, float* reward, uint8_t* done,
                   void* stream);

/* Multi-GPU (no reference counterpart: the reference is one env per process).  Envs shard by index, one process
 * per GPU; the one exchange of the path is the learner-side all-gather of every rank's packed (obs, reward, done) record
 * each step.  These entry points enqueue it from C -- through torch.distributed the same loop body costs the host more
 * than the step costs the GPU at 512 envs per rank.  RCCL is bound with dlopen at the first call (the librccl.so the
 * process has loaded, or ROCm's); a process that never calls them needs no RCCL.
 *   crafter_exchange_unique_id  rank 0 draws the communicator id (ncclGetUniqueId) and hands the 128 bytes to every rank
 *                               (any side channel: torch.distributed broadcast, MPI, a file)
 *   crafter_exchange_create     every rank, collectively (ncclCommInitRank); slots = records in flight (1..8, usually 2)
 *   crafter_step_exchange       crafter_step with its outputs INSIDE `send` -- obs at byte 0 (with_obs), reward at off_reward
 *                               (4-byte aligned), done at off_done -- then ncclAllGather(send -> recv[world][record_bytes]) on
 *                               the exchange's own stream, ordered behind the step's kernels by an event: it overlaps the
 *                               next step.  Before the kernels overwrite `send` the call makes `stream` wait for the slot's
 *                               previous gather.  send / recv: device memory, distinct per slot, caller-owned.
 *   crafter_exchange_wait       `stream` waits for the slot's gather (before anything reads recv)
 * All return 0 or 1 + crafter_exchange_error (thread-local text for the two calls without an exchange).
 * STATUS: exercised with ONE rank only so far (one GPU per test box; tests/test_gpu_dist.py).  A caller with more ranks should
 * check its first gather against a collective it trusts, as bench.py does (the first step's record against
 * torch.distributed.all_gather_into_tensor on every rank, falling back to crafter_amd.dist.StepExchange if any rank disagrees). */
typedef struct crafter_exchange crafter_exchange;
int crafter_exchange_unique_id(uint8_t id[128]);
int crafter_exchange_create(const uint8_t id[128], int32_t rank, int32_t world, int32_t slots, crafter_exchange** out);
void crafter_exchange_destroy(crafter_exchange* x);
int crafter_step_exchange(crafter_handle* h, crafter_exchange* x, int32_t slot, const int32_t* actions, uint8_t* send, uint8_t* recv,
                          int64_t record_bytes, int64_t off_reward, int64_t off_done, int32_t with_obs, void* stream);
int crafter_exchange_wait(crafter_exchange* x, int32_t slot, void* stream);
const char* crafter_exchange_error(const crafter_exchange* x);

/* Diagnostics (no reference counterpart): the order in which the next crafter_step dispatches the envs -- those whose next
 * step draws a night frame or balances the chunks first -- into host int32[num_envs]; synchronises the device.
 * Returns 2 when the handle keeps no order (few envs, no auto-reset, CRAFTER_ORDER=0). */
int crafter_debug_dispatch_order(crafter_handle* h, int32_t* out);
/* Experiments: dispatch in the caller's order (device int32[num_envs], must be a permutation and stay alive) until called
 * with NULL.  Returns 2 when the handle keeps no order. */
int crafter_debug_set_dispatch_order(crafter_handle* h, const int32_t* order);

/* Replaces Env.render() at the configured size (env.py:120-130) for masked envs (NULL: all):
 * re-draws the current frame into out (same layout as obs) and, exactly like the reference,
 * draws the night noise from each env's RNG again (engine.py:208-209). */
int crafter_render(crafter_handle* h, const uint8_t* mask, uint8_t* out, void* stream);

/* The symbolic observation of the state the frame depicts (no reference counterpart as a call; every value is the reference's),
 * for masked envs (NULL: all; rows with a zero mask byte are left untouched).  Either output may be NULL.
 *   local: uint8 [num_envs][2][local_gw][local_gh], indexed [env][plane][x][y].  Local cell (x, y) is world cell
 *     player.pos + (x, y) - (local_gw / 2, local_gh / 2) (engine.py:155-187, LocalView).  Plane 0: the value info['semantic']
 *     has there (engine.py:251-264, SemanticView: the material id, or n_materials + 1 + class index where an object stands),
 *     0 outside the world.  Plane 1: the sprite variant of the object on the cell (objects.py:85-93, 361-367, 395-403) --
 *     player 1 left, 2 right, 3 up, 4 down, 5 sleeping; arrow 1 .. 4 likewise; plant 1 if ripe (grown > 300); otherwise 0.
 *   stats: float [num_envs][n_items + 4]: the inventory in item order (env.py:108-115), facing x, facing y, sleeping (0 / 1)
 *     and the daylight of the env's step (env.py:135-139: the table's double rounded to float).
 * Read-only: unlike crafter_render it draws nothing from the env's RNG and changes no byte of state.  Reads live rows only:
 * no wait for the world pool.  Additive under ABI revision 7: a binding looks it up by name. */
int crafter_symbolic(crafter_handle* h, const uint8_t* mask, uint8_t* local, float* stats, void* stream);

/* The legal-action mask of the state as it stands (no reference counterpart as a call; every value is the reference's), for
 * masked envs (NULL: all; rows with a zero mask byte are left untouched).
 *   legal: uint8 [num_envs][n_actions], required, in the action order of the uploaded rules (crafter_rules.action_kind / _arg).
 *     legal[e][a] = 1 iff Player.update (objects.py:99-131), run on env e's current state with action a, passes every guard of
 *     that action's branch.  target = pos + facing; (material, obj) = world[target], (None, None) outside the world;
 *     awake = not (sleeping and energy < max) (objects.py:103-108; a sleeping player with full energy wakes up and its action
 *     counts normally):
 *       noop     always
 *       move_*   (objects.py:174-179, 36-47) awake, and the destination cell is inside the world, holds no object and its
 *                material is in player_walkable_mask: legal iff the player's position would change (a blocked move still
 *                turns the player and is NOT legal)
 *       do       an object on target (objects.py:181-212): awake, and it is a zombie, skeleton or cow, or a plant with
 *                grown > 300 (an arrow or an unripe plant gives 0); none (objects.py:214-229): awake, and material is water or
 *                collect[material].valid with every `require` amount in the inventory (the `probability` draw is no guard)
 *       sleep    (objects.py:117-119) not sleeping and energy < max
 *       place_*  (objects.py:231-249) awake, no object on target, where_mask has material's bit, every `uses` amount in the
 *                inventory
 *       make_*   (objects.py:251-261) awake, nearby_mask within the materials of World.nearby(pos, 1), every `uses` amount in
 *                the inventory; the window has numpy's slice semantics (engine.py:95-98): EMPTY when x == 0 or y == 0, clipped
 *                at W - 1 / H - 1
 *     For every action but a move, legal == 0 means the step does exactly what noop does (map, objects, inventory,
 *     achievements, counters, RNG stream).  The guards are read from the uploaded crafter_rules.  The state is read as it
 *     stands: no special treatment of a dead player or of a finished env without auto-reset.
 * Read-only: no draw from the env's RNG, no byte of state changes.  Reads live rows only: no wait for the world pool.  Only
 * enqueues work; returns 0, or non-zero with crafter_last_error (legal == NULL is an error).  Additive under ABI revision 7:
 * a binding looks it up by name. */
int crafter_legal_actions(crafter_handle* h, const uint8_t* mask, uint8_t* legal, void* stream);

/* crafter_step on a handle with cfg->auto_reset that also reports, for every env whose `done` byte this step sets, the last
 * observation of the episode that finished -- what the reference's Env.step returns with done=True before the caller resets
 * (Gymnasium / SB3: final_observation / terminal_observation):
 *   final_obs:   uint8 [num_envs][size_h][size_w][3]: env.py:96, self._obs() on the terminal state, with the night noise drawn
 *                from the FINISHED episode's RNG as the reference draws it (engine.py:208-209; the next episode reseeds,
 *                env.py:74).  May be NULL; ignored on a handle that draws no frames (cfg->render_obs == 0).
 *   terminated:  uint8 [num_envs], required: 1 if the player died (env.py:106-115, discount == 0), 0 if the episode only ran
 *                into `length`; 1 when both happen.
 *   final_local, final_stats: crafter_symbolic's pair of the terminal state (layouts above; the daylight entry is that of the
 *                terminal step).  Either may be NULL.
 * Rows of envs that did not finish in this step are NOT touched: read all four under `done`.  obs, reward, done, the terminal
 * rows, info['semantic'], every byte of env state after the call and the worlds later episodes get are bit-identical to
 * crafter_step's; calls of crafter_step, crafter_step_final and crafter_step_n may be mixed freely on one handle.  The step
 * kernels hand every finished env to a second kernel behind the step launch, which draws the terminal frame, then takes the
 * env's next world from the pool or regenerates it inline.  On a handle without auto_reset the call fails (there `obs`
 * already is the final frame).  crafter_step_n and crafter_step_exchange have no final variant.
 * Additive under ABI revision 7: a binding looks it up by name. */
int crafter_step_final(crafter_handle* h, const int32_t* actions, uint8_t* obs, float* reward, uint8_t* done,
                       uint8_t* final_obs, uint8_t* terminated, uint8_t* final_local, float* final_stats, void* stream);

/* crafter_step for a chosen subset of the batch (no reference counterpart: the reference is one env per process; a tree search
 * that stepped scratch rows of a batch, or an actor loop that steps whichever envs have an action ready, would otherwise step
 * every other env too).
 *   idx:     device int32[n], 1 <= n <= num_envs: the envs to step.  Every entry in range, no env named twice.
 *   actions: device int32[n]: actions[i] is the action of env idx[i].
 *   obs, reward, done: the layout of crafter_step -- full [num_envs] rows; obs may be NULL.
 * For every named env the call is exactly crafter_step for that env: its state, its obs / reward / done row, its terminal row,
 * info['semantic'], the auto-reset from the pool or through the regeneration kernel behind the launch, and its requests to the
 * pool.  Rows of envs that are not named are neither read nor written, in the bound state or in obs / reward / done.
 * n == 0 returns 0 and enqueues nothing; idx == NULL, n < 0 and n > num_envs are errors (crafter_last_error).
 * The index list is checked on the device before any env steps, like the copy calls' indices: an entry out of range or an env
 * named twice (two workgroups would step it at once) refuses the WHOLE call -- no row changes -- and sets CRAFTER_ST_BAD_COPY in
 * the status of the named rows that exist (row 0 if none exists).
 * The launch is n workgroups, each fetching its env from idx: it costs what a batch of n envs costs, plus the one-workgroup
 * check in front of it.  crafter_step, crafter_step_envs, crafter_step_final, crafter_step_n and the
 * copy calls may be mixed freely on one handle.  On a handle that keeps a dispatch order the subset launch follows none and
 * builds none; it keeps the named envs' entries of the order's input current.
 * World pool: one call counts as ONE step of the pool's batch period, however few envs it names.  An env steps at most once per
 * call, so the pool's latency assumption -- every env's worlds are requested two episodes ahead -- holds in that env's own
 * steps: a loop of small subsets launches batches more often per env-step than a loop of full steps, never less often.
 * crafter_set_timing attaches its events to this launch as to a step (step time: from the check's start to the subset kernel's
 * end).  There is no `final` variant and no exchange variant of this call.
 * Additive under ABI revision 7: a binding looks it up by name. */
int crafter_step_envs(crafter_handle* h, const int32_t* idx, int32_t n, const int32_t* actions,
                      uint8_t* obs, float* reward, uint8_t* done, void* stream);

/* crafter_step_n for a chosen subset of the batch, with COMPACT outputs (no reference counterpart: a Monte-Carlo playout, a
 * random-shooting planner or an action repeat over the scratch rows of a large batch would otherwise pay `steps` calls of
 * crafter_step_envs, or roll out every env of the batch).
 *   idx:     device int32[n], 1 <= n <= num_envs: the envs to roll out.  Every entry in range, no env named twice, any order.
 *   actions: device int32[steps][n]: actions[t][i] is the action of env idx[i] at its step t.
 *   reward:  device float[steps][n];  done: device uint8[steps][n];
 *   obs:     device uint8[steps][n][size_h][size_w][3] or NULL.  Row i of every output belongs to env idx[i].
 * For every named env the call is exactly `steps` consecutive calls of crafter_step_envs that name it: its state, each step's
 * obs / reward / done, its terminal row, info['semantic'], the auto-reset from the pool or through the regeneration kernel
 * behind the launch, its requests to the pool, level tables, crafter_reseed and authored worlds in progress.  Rows of envs
 * that are not named are neither read nor written, in the bound state or anywhere else.  (As between crafter_step and
 * crafter_step_n, "its state" is every byte a reader of the state looks at: the FREE records of the slot table behind the
 * env's nobj keep whatever was last stored there, and the table goes back to global memory once per launch here.)
 * n == 0 returns 0 and enqueues nothing; idx == NULL, n < 0, n > num_envs, steps < 1 and NULL actions / reward / done are
 * errors (crafter_last_error).
 * The index list is checked on the device before any env steps, as for crafter_step_envs: a bad list refuses the WHOLE call
 * -- no state row and no output byte changes -- and sets CRAFTER_ST_BAD_COPY in the status of the named rows that exist (row 0
 * if none exists).
 * One launch of n workgroups covers the steps up to the world pool's next generation batch, or 16 steps when the pool is off,
 * exactly as crafter_step_n splits its call; each env's state stays in LDS over the steps of a launch.  The call counts as
 * `steps` steps of the pool's batch period.  It may be mixed freely with crafter_step, crafter_step_envs, crafter_step_final,
 * crafter_step_n and the copy calls.  On a handle that keeps a dispatch order it follows none and builds none; it keeps the
 * named envs' entries of the order's input current.  crafter_set_timing attaches its events per launch, as for crafter_step_n.
 * There is no `final` variant and no exchange variant of this call.
 * Additive under ABI revision 7: a binding looks it up by name. */
int crafter_step_n_envs(crafter_handle* h, const int32_t* idx, int32_t n, int32_t steps, const int32_t* actions,
                        uint8_t* obs, float* reward, uint8_t* done, void* stream);

/* Level selection (no reference counterpart as a call: the reference fixes the seed in Env.__init__, env.py:32, and a world is a
 * pure function of (seed, episode), env.py:74).  For every env whose mask byte is non-zero (mask == NULL: all):
 *   rec.seed_lane = seed_lane[i];  rec.episode = max(episode[i], 1) - 1;
 *   both of its world-pool entries are emptied (pool_hdr[0|1][i].ready = 0, .pending = 0);  gen_latest[i] = rec.episode.
 * All pointers are DEVICE pointers.  mask: uint8 [num_envs] or NULL.  seed_lane: uint64 [num_envs], required: CPython's
 * hash(seed) as an unsigned 64-bit lane, what crafter_env_rec.seed_lane holds.  episode: int32 [num_envs], or NULL for 1; values
 * below 1 are taken as 1, and a caller keeps them <= 2^31 - 3 (the pool asks for episode + 2).  Rows with a zero mask byte are not
 * touched and their seed_lane / episode entries are not read.
 * Meaning: the env's NEXT reset -- crafter_reset or the automatic one -- starts episode episode[i] of that seed, exactly what a
 * freshly constructed crafter.Env(seed=...) produces at its episode[i]-th reset(), and every later episode follows from there.
 * The episode in progress plays on unchanged; only its number reads episode[i] - 1 from then on (info['episode'], the
 * `terminal` row's episode entry).
 * Like every other entry point the call only enqueues work.  Before the kernel runs the world pool is brought to rest as before
 * crafter_load_envs: the requests collected so far are launched as a batch and the stream waits (on the device) for every batch
 * launched -- otherwise a batch in flight could deliver a world of the old seed into an emptied entry.  The env regenerates its next
 * world inline once and the pool takes over again.  With the pool off, failed or absent only the record is written (a failed
 * pool's entries, still bound, are emptied too).
 * Additive under ABI revision 7: a binding looks it up by name. */
int crafter_reseed(crafter_handle* h, const uint8_t* mask, const uint64_t* seed_lane, const int32_t* episode, void* stream);

/* Level sets (no reference counterpart: Procgen's num_levels protocol, level replay, a curriculum -- training on a fixed set of K
 * levels under auto-reset without a host round trip per finished env).  A handle may hold a LEVEL TABLE: n_levels entries
 * (seed_lane[j], episode[j] >= 1), 1 <= n_levels <= 65536, optional cumulative weights cum[j] and a 64-bit key.  While a table is
 * set, the reset that takes an env into its k-th episode (k = rec.episode + 1, counted as always: crafter_reset, the automatic
 * reset, a world from the pool or one regenerated inline) generates the world of table entry j = pick(rec.seed_lane, k): its seed is
 * world_seed(seed_lane[j], episode[j]) in place of world_seed(rec.seed_lane, k), and nothing else changes.  rec.seed_lane and
 * rec.episode keep their values and meaning -- the env's draw lane and its reset count (info['episode'], the terminal row) -- and
 * the episode played is, bit for bit, the one a fresh crafter.Env(seed) shows at its episode[j]-th reset().
 * pick, all arithmetic mod 2^64:
 *   z = seed_lane + 0x9E3779B97F4A7C15 * (uint64)k + key
 *   z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z = z ^ (z >> 31);  u = z >> 32
 *   cum == NULL (uniform):  j = (u * n_levels) >> 32
 *   weighted:               j = first index with cum[j] > u   (cum non-decreasing; cum[n_levels - 1] counts as 2^32 whatever
 *                           it holds; a level of weight 0 -- cum[j] == cum[j - 1], or cum[0] == 0 -- is not drawn)
 * A host turns weights w into cum[j] = min(floor(2^32 * sum(w[:j + 1]) / sum(w)), 2^32 - 1).  (Under that clamp one value of u in
 * 2^32, u = 2^32 - 1, falls to the LAST entry whatever its weight.)
 * crafter_set_levels: all pointers are DEVICE pointers -- seed_lane uint64 [n_levels], episode int32 [n_levels] (a value below 1 is
 * taken as 1; a caller keeps them <= 2^31 - 3), cum uint32 [n_levels] or NULL.  The call only enqueues: a kernel copies the table
 * into a buffer the handle owns (allocated once, at the capacity of 65536 entries), so the caller's arrays are free again once
 * the stream has passed the call.  n_levels == 0 clears the table: from each env's next reset on every world is
 * world_seed(rec.seed_lane, k) again; a handle that never sets a table behaves exactly as one of a library without these calls.
 * Errors (crafter_last_error): n_levels outside 0 .. 65536; NULL seed_lane or episode with n_levels > 0.
 * Episodes in progress are not disturbed: a new table takes effect at each env's next reset.  The world pool's entries all hold
 * worlds of the table being replaced: the pool is brought to rest as before crafter_reseed and the same kernel empties EVERY
 * env's two entries and sets gen_latest[env] = rec.episode (no record is edited); each env then regenerates its next world inline
 * once and the pool takes over.  With the pool off, failed or absent only the table is written.
 * Copies (crafter_copy_envs / _save_envs / _load_envs) carry lane and k, so a copy plays the levels its source would, and a store
 * loaded under another table follows that table.  crafter_reseed, with a table set, chooses an env's POSITION in its draw
 * sequence, not its level: held-out evaluation on the same handle clears the table first.
 * crafter_level_ids: ids int32 [num_envs] (device), one thread per env, read-only, no wait for the pool:
 *   ids[env] = pick(rec.seed_lane, rec.episode) under the table in force;  -1 in every row when no table is set;
 * rows with a zero mask byte (mask uint8 [num_envs] or NULL: all) are untouched.  That is the level of the env's episode in
 * progress IF THAT EPISODE BEGAN WHILE THIS TABLE WAS SET (an episode begun under an earlier table, or before a crafter_reseed,
 * reads what the present table and record say, not what it plays).  The exact use: after a step, the ids of the rows with
 * done != 0 are the levels of the episodes that just began.
 * Additive under ABI revision 7: a binding looks them up by name. */
int crafter_set_levels(crafter_handle* h, const uint64_t* seed_lane, const int32_t* episode,
                       const uint32_t* cum, int32_t n_levels, uint64_t key, void* stream);
int crafter_level_ids(crafter_handle* h, const uint8_t* mask, int32_t* ids, void* stream);

/* Measurement aid (no reference counterpart): when enabled, crafter_step attaches HIP start / stop events to
 * its two kernels (hipExtLaunchKernelGGL: the kernels' own execution time on the launch stream, what a
 * profiler reports).  crafter_get_timing waits for the recorded events, returns the SUM of step-kernel and
 * auto-reset-kernel durations in ms over `launches` calls and clears them. */
int crafter_set_timing(crafter_handle* h, int enable);
int crafter_get_timing(crafter_handle* h, double* step_ms, double* reset_ms, int32_t* launches);

/* World pool (no reference counterpart: Env.reset's worldgen, worldgen.py:10-18, runs ahead of time on side
 * streams so that an auto-reset adopts a finished world).  Returns 0 = pool off (no auto-reset / gen_period < 0),
 * 1 = running, 2 = disabled after a HIP error in its scheduler (text in crafter_pool_error; stepping stays
 * correct, finished envs regenerate inline), -1 = null handle.  launched / trusted (may be NULL): generation
 * batches launched so far / known complete. */
int crafter_pool_status(const crafter_handle* h, uint32_t* launched, uint32_t* trusted);
const char* crafter_pool_error(const crafter_handle* h);

/* Unit-test access (no reference counterpart) to the arithmetic the world generator evaluates on the device, so that it
 * can be compared bit for bit with the CPU oracle: mode 0: out[i] = noise3(x[i], y[i], z[i]) of the OpenSimplex instance
 * whose permutation is perm[256] (the third-party opensimplex package behind worldgen.py:11,84-87); mode 1:
 * out[i] = 1 / (1 + exp(-x[i])) (worldgen.py:27) with the library's pinned, correctly rounded exponential (np.exp is a
 * different function on different hosts: csrc/worldgen.hpp exp_cr); mode 2: out[i] = 4 - sqrt(x[i]) (worldgen.py:25);
 * mode 3: out[i] = exp_cr(x[i]).  All pointers are device pointers; perm / y / z may be NULL for modes 1 to 3.  Errors are reported through crafter_last_error(NULL). */
int crafter_debug_eval(int mode, const uint8_t* perm, const double* x, const double* y, const double* z, double* out,
                       int64_t n, void* stream);

/* Last error text of this handle (or of the failed crafter_create when h == NULL). */
const char* crafter_last_error(const crafter_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* CRAFTER_HIP_H_ */
