// The kernels' names for the plain-data types of the C ABI.  The layouts, constants and enum values are stated once, in
// include/crafter_hip_types.h (C99, with every field's meaning): this file includes it and gives the structs and values
// the short names the gfx950 kernels and the host-side harnesses use.  What is defined here is the library's own:
// TablePtrs, the rules head and the compiled-in default rules.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/crafter_hip_types.h"

namespace crafter {

using Obj = crafter_obj;
using ItemList = crafter_item_list;
using CollectRule = crafter_collect_rule;
using PlaceRule = crafter_place_rule;
using MakeRule = crafter_make_rule;
using Rules = crafter_rules;
using Config = crafter_config;
using EnvRec = crafter_env_rec;
using PoolHdr = crafter_pool_hdr;
using StatePtrs = crafter_state_ptrs;
static_assert(sizeof(Obj) == 16, "Obj must be 16 bytes");
static_assert(sizeof(PoolHdr) == 32, "PoolHdr must be 32 bytes");

constexpr int MT_N = CRAFTER_MT_N;
constexpr int MT_M = 397;
constexpr int CHUNK = CRAFTER_CHUNK;
constexpr int MAX_ITEMS = CRAFTER_MAX_ITEMS;
constexpr int MAX_ACH = CRAFTER_MAX_ACH;
constexpr int MAX_MATERIALS = CRAFTER_MAX_MATERIALS;
constexpr int MAX_ACTIONS = CRAFTER_MAX_ACTIONS;
constexpr int MAX_PLACE = CRAFTER_MAX_PLACE;
constexpr int MAX_MAKE = CRAFTER_MAX_MAKE;
constexpr int MAX_USES = CRAFTER_MAX_USES;

// The header's enums are plain C ones; here every value gets its short name in an enum of fixed underlying type, the width
// the kernel code stores and compares it at.
enum : uint8_t {
  T_NONE = CRAFTER_T_NONE, T_PLAYER = CRAFTER_T_PLAYER, T_COW = CRAFTER_T_COW, T_ZOMBIE = CRAFTER_T_ZOMBIE,
  T_SKELETON = CRAFTER_T_SKELETON, T_ARROW = CRAFTER_T_ARROW, T_PLANT = CRAFTER_T_PLANT
};
enum : uint8_t {
  A_NOOP = CRAFTER_A_NOOP, A_MOVE = CRAFTER_A_MOVE, A_DO = CRAFTER_A_DO, A_SLEEP = CRAFTER_A_SLEEP,
  A_PLACE = CRAFTER_A_PLACE, A_MAKE = CRAFTER_A_MAKE
};
enum : uint32_t {
  ST_OBJ_OVERFLOW = CRAFTER_ST_OBJ_OVERFLOW, ST_BAD_ACTION = CRAFTER_ST_BAD_ACTION,
  ST_STEP_OVERFLOW = CRAFTER_ST_STEP_OVERFLOW, ST_CHUNK_OVERFLOW = CRAFTER_ST_CHUNK_OVERFLOW,
  ST_POOL_MISMATCH = CRAFTER_ST_POOL_MISMATCH, ST_PIPE_STALL = CRAFTER_ST_PIPE_STALL, ST_BAD_COPY = CRAFTER_ST_BAD_COPY
};
enum : int32_t {   // texture slots inside tex_tile
  TEX_UNKNOWN = CRAFTER_TEX_MATERIAL0,
  TEX_MATERIAL0 = CRAFTER_TEX_MATERIAL0, TEX_PLAYER_LEFT = CRAFTER_TEX_PLAYER_LEFT,
  TEX_PLAYER_RIGHT = CRAFTER_TEX_PLAYER_RIGHT, TEX_PLAYER_UP = CRAFTER_TEX_PLAYER_UP,
  TEX_PLAYER_DOWN = CRAFTER_TEX_PLAYER_DOWN, TEX_PLAYER_SLEEP = CRAFTER_TEX_PLAYER_SLEEP, TEX_COW = CRAFTER_TEX_COW,
  TEX_ZOMBIE = CRAFTER_TEX_ZOMBIE, TEX_SKELETON = CRAFTER_TEX_SKELETON, TEX_ARROW_LEFT = CRAFTER_TEX_ARROW_LEFT,
  TEX_ARROW_RIGHT = CRAFTER_TEX_ARROW_RIGHT, TEX_ARROW_UP = CRAFTER_TEX_ARROW_UP, TEX_ARROW_DOWN = CRAFTER_TEX_ARROW_DOWN,
  TEX_PLANT = CRAFTER_TEX_PLANT, TEX_PLANT_RIPE = CRAFTER_TEX_PLANT_RIPE, TEX_COUNT = CRAFTER_TEX_COUNT
};

// The scalars and small tables every object update reads (walkable masks, material / item ids, ...): the part of
// Rules in front of the collect / place / make tables.  The kernels keep a copy of it in LDS: through the global
// pointer each access is a vector load from memory (~700 clk on the rule code's critical path).
#define CRAFTER_RULES_HEAD_BYTES ((int)((offsetof(crafter::Rules, collect) + 15) / 16 * 16))

// The compiled rules of the baked data.yaml as constants (tools/bake_default_rules.py): the step kernel has an
// instance that reads its rules from here, so that material / item ids, masks and limits fold into the code.
struct alignas(8) DefaultRulesWords {
  uint32_t w[sizeof(Rules) / 4];
};
static constexpr DefaultRulesWords kDefaultRules = {{
#include "default_rules.inc"
}};
// action_kind / action_arg of the default rules as two packed literals, 3 bits per action: the one table the rule code
// indexes with a run-time value on EVERY step -- through kDefaultRules that is a load from global memory (plus a wait
// for everything else in flight) at the head of the serial rule phase; from a literal it is a scalar shift and mask.
constexpr int kPackedActions = 21;   // 63 bits
__host__ __device__ constexpr uint32_t default_rules_byte(int off) { return (kDefaultRules.w[off / 4] >> (8 * (off % 4))) & 0xFFu; }
__host__ __device__ constexpr bool default_actions_pack(int field_off) {
  for (int a = 0; a < MAX_ACTIONS; a++)
    if (default_rules_byte(field_off + a) >= (a < kPackedActions ? 8u : 1u)) return false;
  return true;
}
__host__ __device__ constexpr uint64_t default_actions_packed(int field_off) {
  uint64_t v = 0;
  for (int a = 0; a < kPackedActions; a++) v |= (uint64_t)default_rules_byte(field_off + a) << (3 * a);
  return v;
}
static_assert(default_actions_pack(offsetof(Rules, action_kind)) && default_actions_pack(offsetof(Rules, action_arg)),
              "default action table does not fit 3 bits x 21 actions");
// item_max of the default rules, 4 bits per item: the per-step inventory clamp (objects.py:126-128) reads it per lane
__host__ __device__ constexpr uint32_t default_rules_word(int off) { return kDefaultRules.w[off / 4]; }
__host__ __device__ constexpr bool default_item_max_packs() {
  for (int i = 0; i < MAX_ITEMS; i++)
    if (default_rules_word(offsetof(Rules, item_max) + 4 * i) >= 16u) return false;
  return MAX_ITEMS <= 16;
}
__host__ __device__ constexpr uint64_t default_item_max_packed() {
  uint64_t v = 0;
  for (int i = 0; i < MAX_ITEMS && i < 16; i++) v |= (uint64_t)default_rules_word(offsetof(Rules, item_max) + 4 * i) << (4 * i);
  return v;
}
static_assert(default_item_max_packs(), "default item limits do not fit 4 bits x 16 items");
constexpr uint64_t kDefaultItemMax = default_item_max_packed();
constexpr uint64_t kDefaultActionKinds = default_actions_packed(offsetof(Rules, action_kind));
constexpr uint64_t kDefaultActionArgs = default_actions_packed(offsetof(Rules, action_arg));

// Library-owned read-only tables (uploaded once per handle).
struct TablePtrs {
  const Rules* rules;
  const uint8_t* atlas;        // RGBA texels, [x][y] order per texture
  const int32_t* tex_tile;     // [n_tex]  byte offset of each unit-sized texture, -1 if absent
  const int32_t* tex_icon;     // [MAX_ITEMS] byte offset of each item icon
  const int32_t* tex_digit;    // [11] digits '1'..'9' at [1..9], 'unknown' at [10]
  const uint8_t* tex_alpha;    // [n_tex + MAX_ITEMS + 11] 1 if the source PNG had an alpha channel
  const int32_t* item_pos;     // [MAX_ITEMS][4] icon x,y and digit x,y inside the item view
  const double* daylight;      // [n_daylight] env.py:135-139 evaluated by numpy on the host
  const double* vignette;      // [local_w][local_h] engine.py:213-218 evaluated by numpy
  const float* unit255;        // [256] float32(i) / float32(255)  (engine.py:279-281)
  const uint8_t* render_static;  // the renderer's static LDS block (render.hpp render_static_bytes), built once by
                                 // Renderer::build_static when the tables are uploaded
};

}  // namespace crafter
