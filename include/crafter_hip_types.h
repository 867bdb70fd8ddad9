/* libcrafter_hip.so -- the plain-data structs that cross the C ABI of crafter_hip.h, in C99.
 *
 * Everything a binding in C / Rust / Go / Java needs to fill the constructor arguments of the reference
 * (crafter.Env.__init__, env.py:27-56) and to read the state back: no C++, fixed-width integers, doubles and pointers
 * only (the Python binding fills the structs through ctypes, crafter_amd/tables.py).
 * This file is the ONE statement of these layouts, constants and enums: the gfx950 kernels are compiled against it too
 * (crafter_amd/csrc/types.hpp only gives the structs and values their short C++ names), so what a binding reads here is
 * what the device code uses.  crafter_amd/abi.py is the ctypes / numpy mirror; tests/test_host_logic.py compares every
 * offset, size and value of it with this file.
 */
#ifndef CRAFTER_HIP_TYPES_H_
#define CRAFTER_HIP_TYPES_H_

#include <stddef.h>
#include <stdint.h>

#define CRAFTER_MT_N 624          /* words of an MT19937 key (numpy RandomState)                    */
#define CRAFTER_CHUNK 12          /* chunk size (12, 12), env.py:40                                 */
#define CRAFTER_MAX_ITEMS 16      /* data.yaml items (16 in the reference)                          */
#define CRAFTER_MAX_ACH 32        /* data.yaml achievements (22 in the reference)                   */
#define CRAFTER_MAX_MATERIALS 16
#define CRAFTER_MAX_ACTIONS 32
#define CRAFTER_MAX_PLACE 8
#define CRAFTER_MAX_MAKE 8
#define CRAFTER_MAX_USES 4

/* object classes, in the order of the reference's SemanticView list (env.py:47-49), so the semantic id of an object is
 * n_materials + class */
enum { CRAFTER_T_NONE = 0, CRAFTER_T_PLAYER = 1, CRAFTER_T_COW = 2, CRAFTER_T_ZOMBIE = 3, CRAFTER_T_SKELETON = 4,
       CRAFTER_T_ARROW = 5, CRAFTER_T_PLANT = 6 };
/* action kinds (data.yaml action names are decoded on the host, objects.py:109-123) */
enum { CRAFTER_A_NOOP = 0, CRAFTER_A_MOVE = 1, CRAFTER_A_DO = 2, CRAFTER_A_SLEEP = 3, CRAFTER_A_PLACE = 4, CRAFTER_A_MAKE = 5 };
/* sticky per-env status bits (crafter_env_rec.status): the product fails loudly on any of these
 *   OBJ_OVERFLOW    object table capacity exceeded
 *   BAD_ACTION      action index out of range (reference: IndexError, env.py:86)
 *   STEP_OVERFLOW   step beyond the uploaded daylight table
 *   CHUNK_OVERFLOW  chunk table capacity exceeded
 *   POOL_MISMATCH   a pooled world trusted by the scheduler did not hold the episode it was adopted for
 *   PIPE_STALL      a bounded in-kernel wait ran out (no kernel of this build waits inside a launch: reserved; the
 *                   pipelined step kernel that set it was removed in round 5)
 *   BAD_COPY        crafter_copy_envs / _save_envs / _load_envs refused its indices (out of range, a destination named
 *                   twice, or one that is also a source): nothing was copied */
enum { CRAFTER_ST_OBJ_OVERFLOW = 1, CRAFTER_ST_BAD_ACTION = 2, CRAFTER_ST_STEP_OVERFLOW = 4, CRAFTER_ST_CHUNK_OVERFLOW = 8,
       CRAFTER_ST_POOL_MISMATCH = 16, CRAFTER_ST_PIPE_STALL = 32,
       CRAFTER_ST_BAD_COPY = 64 };
/* the parts of a state fingerprint (crafter_hip_fingerprint.h): bit p of a part mask is part p, and part p's hash is
 * column p of part_hash.  VISIBLE: what a frame depicts; DYNAMICS: every part but IDENT -- two envs with equal DYNAMICS keys
 * are meant to produce identical outputs under any common action sequence until the episode ends */
#define CRAFTER_FP_PARTS 7
enum { CRAFTER_FP_MAP = 1, CRAFTER_FP_OBJECTS = 2, CRAFTER_FP_PLAYER = 4, CRAFTER_FP_CLOCK = 8, CRAFTER_FP_RNG = 16,
       CRAFTER_FP_CHUNKS = 32, CRAFTER_FP_IDENT = 64,
       CRAFTER_FP_VISIBLE = 1 | 2 | 4, CRAFTER_FP_DYNAMICS = 63, CRAFTER_FP_ALL = 127 };
/* texture slots of crafter_host_tables.tex_tile: material id m at CRAFTER_TEX_MATERIAL0 + m (0 = None -> 'unknown'), then
 * the sprites */
enum { CRAFTER_TEX_MATERIAL0 = 0, CRAFTER_TEX_PLAYER_LEFT = 17, CRAFTER_TEX_PLAYER_RIGHT, CRAFTER_TEX_PLAYER_UP,
       CRAFTER_TEX_PLAYER_DOWN, CRAFTER_TEX_PLAYER_SLEEP, CRAFTER_TEX_COW, CRAFTER_TEX_ZOMBIE, CRAFTER_TEX_SKELETON,
       CRAFTER_TEX_ARROW_LEFT, CRAFTER_TEX_ARROW_RIGHT, CRAFTER_TEX_ARROW_UP, CRAFTER_TEX_ARROW_DOWN, CRAFTER_TEX_PLANT,
       CRAFTER_TEX_PLANT_RIPE, CRAFTER_TEX_COUNT };

#if defined(__GNUC__) || defined(__clang__)
#define CRAFTER_ALIGN16 __attribute__((aligned(16)))
#else
#define CRAFTER_ALIGN16
#endif

/* One world object (engine.py:50-57 World.add): one 16-byte record (one dwordx4 / ds_read_b128). */
typedef struct crafter_obj {
  uint8_t type;      /* CRAFTER_T_*; 0 = free slot                                                  */
  int8_t health;     /* objects.py:25-30 (the player's health lives in the inventory instead)       */
  int8_t fx, fy;     /* facing (player, arrow)                                                      */
  uint16_t x, y;
  int32_t aux;       /* zombie cooldown / skeleton reload / plant grown                             */
  uint32_t pad;
} CRAFTER_ALIGN16 crafter_obj;

typedef struct crafter_item_list {
  int32_t n;
  int32_t item[CRAFTER_MAX_USES];
  int32_t amount[CRAFTER_MAX_USES];
  int32_t ach[CRAFTER_MAX_USES];   /* for 'receive': index of achievement collect_<item>; else -1 */
} crafter_item_list;

typedef struct crafter_collect_rule {   /* data.yaml collect, objects.py:214-229 */
  int32_t valid;
  int32_t leaves;            /* material id written in place of the collected one */
  double probability;        /* default 1 */
  crafter_item_list require;
  crafter_item_list receive;
} crafter_collect_rule;

typedef struct crafter_place_rule {     /* data.yaml place, objects.py:231-249 */
  int32_t valid;
  int32_t is_object;         /* 1: adds a Plant; 0: sets `material` */
  int32_t material;          /* material id written for type 'material' */
  int32_t ach;               /* place_<name> */
  uint32_t where_mask;       /* bit m set: material id m allowed under it */
  int32_t pad;
  crafter_item_list uses;
} crafter_place_rule;

typedef struct crafter_make_rule {      /* data.yaml make, objects.py:251-261 */
  int32_t valid;
  int32_t item;              /* produced item index */
  int32_t gives;
  int32_t ach;               /* make_<name> */
  uint32_t nearby_mask;      /* all of these materials must be in the 3x3 window */
  int32_t pad;
  crafter_item_list uses;
} crafter_make_rule;

/* data.yaml compiled to integers (constants.py:6-8); material ids are 1 + position in data.yaml's list (0 = None).
 * The fields in front of `collect` are the scalars and small tables every object update reads: the kernels keep a copy
 * of that head in LDS (types.hpp CRAFTER_RULES_HEAD_BYTES). */
typedef struct crafter_rules {
  int32_t n_actions, n_materials, n_items, n_achievements;
  uint8_t action_kind[CRAFTER_MAX_ACTIONS];
  uint8_t action_arg[CRAFTER_MAX_ACTIONS];   /* MOVE: dir 0..3 = left, right, up, down; PLACE / MAKE: rule index */
  int32_t item_max[CRAFTER_MAX_ITEMS];
  int32_t item_init[CRAFTER_MAX_ITEMS];
  uint32_t walkable_mask;                    /* data.yaml walkable (objects.py:21-22) */
  uint32_t player_walkable_mask;             /* + lava            (objects.py:96-97) */
  uint32_t arrow_walkable_mask;              /* + water, lava     (objects.py:369-371) */
  uint32_t arrow_breaks_mask;                /* table, furnace    (objects.py:381) */
  int32_t mat_water, mat_grass, mat_stone, mat_path, mat_sand, mat_tree, mat_lava, mat_coal, mat_iron, mat_diamond,
      mat_table, mat_furnace;
  int32_t item_health, item_food, item_drink, item_energy;
  int32_t item_wood_sword, item_stone_sword, item_iron_sword;
  int32_t ach_wake_up, ach_eat_plant, ach_defeat_zombie, ach_defeat_skeleton, ach_eat_cow;
  crafter_collect_rule collect[CRAFTER_MAX_MATERIALS + 1];   /* indexed by material id */
  crafter_place_rule place[CRAFTER_MAX_PLACE];
  crafter_make_rule make[CRAFTER_MAX_MAKE];
} crafter_rules;

/* Static configuration of a batch: crafter.Env(area, view, size, reward, length, seed) (env.py:27-56) for num_envs
 * environments.  Derived fields exactly as the reference computes them:
 *   unit = size // view (env.py:42);  local grid = (view_w, view_h - item_rows), item_rows = ceil(n_items / view_w)
 *   (env.py:43-46);  border = (size - unit * view) // 2 (env.py:127);  icon = int(0.8 * unit), digit = int(0.6 * unit)
 *   (engine.py:239,246);  update_dist = 2 * max(view) (env.py:88);  nchunk = ceil(area / 12). */
typedef struct crafter_config {
  int32_t num_envs;
  int32_t W, H;               /* area                                                                */
  int32_t view_w, view_h;     /* view (9, 9)                                                         */
  int32_t size_w, size_h;     /* obs size (64, 64)                                                   */
  int32_t unit_x, unit_y;     /* size // view                                                        */
  int32_t local_gw, local_gh; /* LocalView grid (9, 7)                                               */
  int32_t item_gw, item_gh;   /* ItemView grid (9, 2)                                                */
  int32_t border_x, border_y; /* env.py:127                                                          */
  int32_t icon_w, icon_h;     /* int(0.8 * unit), engine.py:239                                      */
  int32_t digit_w, digit_h;   /* int(0.6 * unit), engine.py:246                                      */
  int32_t max_objects;        /* capacity C of the object table, slot 0 reserved (256 for 64x64)     */
  int32_t nchunk_x, nchunk_y; /* ceil(W / 12), ceil(H / 12)                                          */
  int32_t length;             /* 0 = None                                                            */
  int32_t update_dist;        /* 2 * max(view), env.py:88                                            */
  int32_t n_daylight;         /* entries of crafter_host_tables.daylight (length + 2)                */
  int32_t auto_reset;         /* 1: a finished env is regenerated inside crafter_step                */
  int32_t want_semantic;      /* 1: info['semantic'] written every step (state.semantic)             */
  int32_t render_obs;         /* 0: no pixels (the night noise is still drawn from the RNG)          */
  int32_t reward;             /* 0: returned reward forced to 0.0 (env.py:116-117)                   */
  int32_t step_threads;       /* 0 or the build's fixed step / render workgroup size (256)           */
  int32_t reset_threads;      /* 0 or the build's fixed reset / generation workgroup size (1024): workgroup sizes are
                               *   compile-time constants of the library, crafter_create refuses anything else */
  int32_t gen_period;         /* world pool: steps between generation batches (0 = default 16, < 0 = pool off) */
} crafter_config;

/* Per-env scalar record kept in HBM between launches: what info[...] of Env.step is read from (env.py:108-115). */
typedef struct crafter_env_rec {
  int32_t mt_pos;             /* MT19937 index, 624 = twist before the next draw                     */
  int32_t step;               /* Env._step                                                           */
  int32_t episode;            /* Env._episode                                                        */
  int32_t nobj;               /* slots in use incl. reserved slot 0 (next free slot)                 */
  uint64_t seed_lane;         /* CPython hash(seed) as an unsigned 64-bit lane (env.py:74)           */
  int32_t nchunks_seen;
  uint32_t status;            /* CRAFTER_ST_* bits, sticky                                           */
  int32_t inv[CRAFTER_MAX_ITEMS];
  int32_t ach[CRAFTER_MAX_ACH];
  int32_t hunger2, thirst2, fatigue2, recover2;   /* 2x fixed point of objects.py:79-82              */
  int32_t player_last_health; /* Player._last_health (objects.py:78)                                 */
  int32_t env_last_health;    /* Env._last_health    (env.py:77)                                     */
  uint32_t unlocked;          /* bitmask over achievements (Env._unlocked)                           */
  int32_t sleeping;
  /* outputs of the latest step (so the N = 1 facade can rebuild exact Python floats) */
  int32_t dhealth;            /* health - last_health (reward numerator, env.py:97)                  */
  uint32_t new_unlocked;      /* achievements unlocked by the latest step                            */
  int32_t dead;
  int32_t done;
  int32_t needs_reset;        /* set by step when auto_reset and done                                */
  /* running totals of the episode (so a finished episode can be reported after an auto-reset) */
  int32_t ep_dhealth;         /* sum of dhealth over the episode's steps                             */
  int32_t ep_unlock_steps;    /* number of steps that unlocked something (+1.0 reward each, env.py:102-104) */
  int32_t pad[1];
} CRAFTER_ALIGN16 crafter_env_rec;

/* Header of one pre-generated world (the world pool, see env_kernels.hpp gen_body / adopt_world): 32 bytes. */
typedef struct crafter_pool_hdr {
  uint64_t ready;             /* (generation batch sequence << 32) | episode the entry holds; one 8-byte store */
  int32_t mt_pos;
  int32_t nobj;
  int32_t nchunks_seen;
  int32_t pad;
  int32_t pending;            /* episode whose generation into this entry has been requested and is not through its
                               *   batch yet (0: none): a second writer of the entry must wait for it
                               *   (request_generation defers) */
  int32_t pad2;
} CRAFTER_ALIGN16 crafter_pool_hdr;

/* Caller-owned DEVICE buffers holding the world state (torch tensors in the Python binding); the library never allocates
 * or frees these.  N = num_envs, cells = W * H, C = max_objects, nch = nchunk_x * nchunk_y.  Zero-filled at allocation
 * except rec[i].seed_lane = hash(seed_i), rec[i].mt_pos = 624, rec[i].nobj = 1.  Buffers marked (pool) are only needed
 * with auto_reset = 1 and gen_period >= 0; semantic only with want_semantic; prof may be NULL.  mat / objmap / objs / mt /
 * rec must be 16-byte aligned.
 * The world pool holds the upcoming worlds of every env, generated ahead of time on side streams: TWO entries per env,
 * indexed by episode parity, so that generations of consecutive episodes (which may run concurrently on different
 * streams) never write the same entry. */
typedef struct crafter_state_ptrs {
  uint8_t* mat;               /* [N][cells]  material ids, index x * H + y (reference _mat_map[x][y])                */
  uint16_t* objmap;           /* [N][cells]  slot id per cell, 0 = empty (reference _obj_map; scratch for LDS-resident
                               *   worlds, crafter_slot_map_derived)                                                 */
  crafter_obj* objs;          /* [N][C]      slot table, slot 0 unused, slot 1 = player                              */
  uint32_t* mt;               /* [N][624]    MT19937 key                                                             */
  crafter_env_rec* rec;       /* [N]                                                                                 */
  uint16_t* chunk_order;      /* [N][nch]    chunk ids in first-touch order (engine.py:36 dict order)                */
  uint8_t* chunk_seen;        /* [N][nch]                                                                            */
  int32_t* census;            /* [N][nch][5] per chunk: grass cells, path cells (kept current on every material write),
                               *   zombies, skeletons, cows (recounted by each balance pass)                         */
  uint8_t* semantic;          /* [N][cells] or NULL                                                                  */
  uint64_t* prof;             /* [N][16] shader-clock stamps: step kernel phases [0..7], reset kernel [8..15]; or NULL */
  int32_t* reset_q;           /* [2][N + 4] per step parity: count (+3 pad) then env ids that must be regenerated    */
  uint8_t* pool_mat;          /* (pool) [2][N][cells]                                                                */
  crafter_obj* pool_objs;     /* (pool) [2][N][C]                                                                    */
  uint32_t* pool_mt;          /* (pool) [2][N][624]  RandomState key right after worldgen                            */
  crafter_pool_hdr* pool_hdr; /* (pool) [2][N]                                                                       */
  uint16_t* pool_chunk_order; /* (pool) [2][N][nch]                                                                  */
  int32_t* gen_q;             /* (pool) [8][4 N + 4] ring of request segments: count (+3 pad) then up to 2 N (env,
                               *   episode) pairs                                                                    */
  int32_t* gen_latest;        /* (pool) [N] episode of the newest generation request of each env                     */
  int32_t* terminal;          /* [N][CRAFTER_MAX_ACH + 4] what a stats recorder needs of an episode that just ended
                               *   (recorder.py:53-66), written at done: achievements[CRAFTER_MAX_ACH], length, sum
                               *   dhealth, unlock steps, episode; or NULL                                           */
  int32_t* pool_stats;        /* (pool) [4] counters since bind: worlds adopted from the pool, envs regenerated inline
                               *   although the pool is on (world not ready in time), -, -; or NULL                  */
  uint8_t* pool_perm;         /* (pool) [2][N][512] OpenSimplex perm[256] | pg3[256] of the world being generated
                               *   (hand-off between the seeding and the classification kernels)                     */
  int32_t* pool_census;       /* (pool) [2][N][nch][5] the pooled world's grass / path cell counts per chunk (the
                               *   creature counts are 0): counted by the generator, so that adopting a world is a
                               *   copy and not a pass over its map                                                  */
} crafter_state_ptrs;

#endif /* CRAFTER_HIP_TYPES_H_ */
