// Everything that computes an LDS size or offset (all __host__ __device__: the kernels and the host that launches them agree by
// construction): the geometry predicates, the env layouts, the frame kernel's and the generation kernels' carve-ups.
#pragma once
#include "env_core.hpp"
#include "render.hpp"
#include "worldgen.hpp"

namespace crafter {

// The geometry everybody uses -- crafter.Env() defaults: 64x64 world, 9x9 view, 64x64 image (env.py:27-46) -- as
// compile-time constants: with GEO = 1 the step kernel overwrites those Config fields with literals, and since
// every helper is inlined into it the compiler folds them everywhere (LDS offsets become immediates, divisions
// by the unit / grid sizes become multiplies, loop trip counts are known).  Any other configuration runs the
// generic instance (GEO = 0) of the same code.
__host__ __device__ inline bool is_default_view(const Config& c);   // (the view's seventeen fields: below)
__device__ __forceinline__ Config with_default_view(Config c);
__host__ __device__ inline bool is_default_geometry(const Config& c) {
  return is_default_view(c) && c.W == 64 && c.H == 64 && c.max_objects == 256 && c.nchunk_x == 6 && c.nchunk_y == 6;
}
__device__ __forceinline__ Config with_default_geometry(Config c) {
  c = with_default_view(c);
  c.W = 64; c.H = 64; c.max_objects = 256; c.nchunk_x = 6; c.nchunk_y = 6;
  return c;
}

// ... and the same for worlds of ANY size seen through crafter.Env()'s default view (9x9 view, 64x64 image; GEO = 2: BASELINE
// configs[3], 256x256): everything about the frame and the update distance folds, the world's extent, its chunk grid and the
// slot table's length stay run-time values.
__host__ __device__ inline bool is_default_view(const Config& c) {
  return c.view_w == 9 && c.view_h == 9 && c.size_w == 64 && c.size_h == 64 && c.unit_x == 7 && c.unit_y == 7 && c.local_gw == 9 &&
         c.local_gh == 7 && c.item_gw == 9 && c.item_gh == 2 && c.border_x == 0 && c.border_y == 0 && c.icon_w == 5 && c.icon_h == 5 &&
         c.digit_w == 4 && c.digit_h == 4 && c.update_dist == 18;
}
__device__ __forceinline__ Config with_default_view(Config c) {
  c.view_w = 9; c.view_h = 9; c.size_w = 64; c.size_h = 64; c.unit_x = 7; c.unit_y = 7;
  c.local_gw = 9; c.local_gh = 7; c.item_gw = 9; c.item_gh = 2; c.border_x = 0; c.border_y = 0; c.icon_w = 5; c.icon_h = 5;
  c.digit_w = 4; c.digit_h = 4; c.update_dist = 18;
  return c;
}

struct LdsLayout {
  int maps_in_lds;   // 1: mat + objmap are staged in LDS; 0: large world, the maps stay in HBM (L2)
  int frame_over_objs = 0;   // the LDS frame extends over the slot table: objs must be stored before the frame is composed
  int mat, objmap, frame, frame_bytes, objs, mt, rec, rules, chunk_order, chunk_seen, census, wg, scratch, render, total;
  int mtb = -1;      // the second MT19937 state (night frames; the worldgen's stream window): inside the wg region
  int far = -1;      // big_layout: the scan's counters, index, record cache and near bits (env_core.hpp FarSlot); the slot table itself stays in global memory
  int total_no_render;   // the renderer's region comes last: kernels that never draw (world-pool generation) launch without it
};

// Worlds whose maps (3 bytes per cell) would push one env's LDS past this stay in HBM.
constexpr int kMaxLdsWithMaps = 96 * 1024;
// The step kernels' compact layout keeps of the worldgen scratch only what a step uses: the second MT19937 state, and in front of
// it the few bytes by which a night frame's pixel buffer (63 x 49 words) outgrows the maps and the slot table it recycles.  Round 6:
// 64 bytes instead of the scratch's first KB -- with the /255 table out of LDS (render.hpp) the default instance's workgroup is
// 24,848 B = 20 LDS granules of 1,280 B instead of 21: six of them leave a CU 8 granules, and a classification workgroup of the
// world pool (6 granules) runs BESIDE them instead of displacing one.
constexpr int kCompactWgHead = 64;
constexpr int kRenderStaticBound = 20 * 1024;   // >= render_static_bytes + sprite_rows_bytes of any accepted frame size

// The run every env layout ends its tables with, from offset o on: MT state | record | staged rules (rules_bytes; 0: none) |
// chunk order | chunk seen | census (census_in_lds false: it stays in global memory, L.census = -1).
__host__ __device__ inline void layout_tail(LdsLayout& L, int& o, const Config& c, int rules_bytes, bool census_in_lds) {
  int nch = c.nchunk_x * c.nchunk_y;
  L.mt = o;           o += align16(4 * MT_N);
  L.rec = o;          o += align16((int)sizeof(EnvRec));
  L.rules = o;        o += rules_bytes;
  L.chunk_order = o;  o += align16(2 * nch);
  L.chunk_seen = o;   o += align16(nch);
  L.census = census_in_lds ? o : -1;
  o += census_in_lds ? align16(20 * nch) : 0;
}
// ... and what closes every layout: the workgroup's scratch words and the renderer's region (render_bytes; 0: none), which comes last
__host__ __device__ inline void layout_end(LdsLayout& L, int o, int render_bytes) {
  L.scratch = o;      o += 16;
  L.total_no_render = o;
  L.render = o;       o += render_bytes;
  L.total = o;
}

// slot_bytes: sizeof of the cell -> slot map's element in THIS kernel's LDS (the map is derived state, every kernel
// rebuilds its own): 2, or 1 for the step kernel's default-geometry instance.
// lean: the rule kernel of the split step (crafter_rules_kernel): no worldgen scratch / second MT state, no renderer region.
// LaneSlots layout (the rule kernel of the default instance, env_core.hpp): a window of the material map, no slot map,
// no staged rules, no worldgen scratch, no renderer region.
__host__ __device__ inline LdsLayout lane_layout(const Config& c) {
  LdsLayout L;
  int o = 0;
  L.maps_in_lds = 1;
  L.mat = o;          o += align16(kWinX * kWinY);
  L.objmap = -1;
  L.frame = 0;
  L.frame_bytes = 0;
  L.objs = o;         o += 16 * c.max_objects;
  L.wg = -1;
  layout_tail(L, o, c, 0, true);   // (rules: the running offset; nothing is staged and nothing reads it here)
  layout_end(L, o, 0);
  return L;
}
__host__ __device__ inline bool lane_layout_ok(const Config& c) {   // the window must fit the map, rows must be 8-byte aligned
  return c.W >= kWinX && c.H >= kWinY && c.H % 8 == 0 && c.max_objects <= 256;
}

// with_rules false: the instance runs the compiled-in rules and stages none (the resident rollout of the default instance:
// 280 bytes that decide whether a sixth workgroup fits a CU)
__host__ __device__ inline LdsLayout lds_layout(const Config& c, int slot_bytes = 2, bool lean = false, bool with_rules = true) {
  LdsLayout L;
  int cells = c.W * c.H;
  int nch = c.nchunk_x * c.nchunk_y;
  // Residency must not depend on the frame size: a render(size) handle (another unit / atlas over the SAME state
  // buffers) has to come to the same decision as the handle that steps, because the slot map of an LDS-resident
  // world is derived state that is never stored.  So the decision prices the renderer's region at a fixed bound
  // (crafter_create rejects frame sizes whose tables exceed it) instead of at render_lds_bytes(c).
  int rest = 16 * c.max_objects + align16(4 * MT_N) + align16((int)sizeof(EnvRec)) + CRAFTER_RULES_HEAD_BYTES + align16(2 * nch) + align16(nch) +
             align16(20 * nch) + render_frame_bytes(c) + kRenderStaticBound + align16(WG_LDS_BYTES) + 16;
  int maps = align16(cells) + align16(slot_bytes * cells);
  // a night frame's pixels wait in LDS, one word each in the noise stream's order (render.hpp), when they fit
  int want_frame = align16(4 * c.local_gw * c.unit_x * c.local_gh * c.unit_y);
  L.maps_in_lds = (align16(cells) + align16(2 * cells) + rest <= kMaxLdsWithMaps) ? 1 : 0;   // same answer for every slot_bytes
  int o = 0;
  if (L.maps_in_lds) {
    L.mat = o;        o += align16(cells);
    L.objmap = o;     o += align16(slot_bytes * cells);
    // the map copies are dead once the per-frame render tables exist: the pixel buffer reuses their LDS -- and, when the
    // maps alone are too small, the slot table behind them, which is then stored to HBM before the frame is drawn
    // (frame_over_objs), and in the step kernel's compact layout the first bytes of the worldgen scratch behind that,
    // which no step uses
    L.frame = 0;
    L.frame_bytes = (!lean && want_frame <= maps + 16 * c.max_objects + (slot_bytes == 1 ? kCompactWgHead : 0)) ? want_frame : 0;
    L.frame_over_objs = L.frame_bytes > maps;
  } else {
    L.mat = L.objmap = -1;
    L.frame = o;
    L.frame_bytes = want_frame <= 16 * 1024 ? want_frame : 0;
    o += L.frame_bytes;
  }
  L.objs = o;         o += 16 * c.max_objects;
  // compact layout (the step kernels): right behind the slot table, and without noise3's tables -- a step only uses the
  // second MT19937 state (night frames) and the first KB (the tail of a night frame's pixel buffer)
  if (slot_bytes == 1) { L.wg = o; L.mtb = o + kCompactWgHead; o += lean ? 0 : kCompactWgHead + align16(4 * MT_N); }
  layout_tail(L, o, c, with_rules ? CRAFTER_RULES_HEAD_BYTES : 0, true);
  if (slot_bytes != 1) { L.wg = o; L.mtb = o + 1024; o += align16(WG_LDS_BYTES); }
  layout_end(L, o, lean ? 0 : align16(render_lds_bytes(c)));
  return L;
}

// The step kernel's layout for worlds whose maps stay in HBM (crafter_step_kernel<0, 0, 0>, the rollout instance of the
// same; 256x256: BASELINE configs[3]).  lds_layout prices such an env at 73 KB -- two step workgroups per CU, the bound of
// configs[3] in round 3 -- of which a step needs neither the night frame's pixel buffer (12.4 KB: the env's
// scratch in global memory, as the frame kernel of the split step keeps it: Renderer::pix_global), nor the census (9.7 KB
// for 484 chunks: Env::census_global), nor noise3's tables in the worldgen scratch (3 KB: a step only uses the second MT
// state).  48.3 KB: three per CU -- until round 6, which took the slot table out as well (32 KB for 2048 slots: it stays in
// global memory, every write goes through to it, and what a step reads of it comes from one scan at stage-in -- env_core.hpp
// FarSlot): 13.1 KB + 2 KB of cache and near bits = 15.1 KB.
__host__ __device__ inline LdsLayout big_layout(const Config& c) {
  LdsLayout L;
  int o = 0;
  L.maps_in_lds = 0;
  L.mat = L.objmap = -1;
  L.frame = 0;
  L.frame_bytes = 0;
  L.frame_over_objs = 0;
  L.objs = -1;
  L.far = o;          o += far_lds_bytes(c.max_objects);
  L.wg = L.mtb = o;   o += align16(4 * MT_N);   // (no pixel buffer in LDS, no worldgen: of the scratch only the second MT state)
  layout_tail(L, o, c, CRAFTER_RULES_HEAD_BYTES, false);
  layout_end(L, o, align16(render_lds_bytes(c)));
  return L;
}

// Env.reset / the regeneration kernel / the fused generation appended to crafter_reset_kernel, for worlds whose maps stay in
// HBM: the slot table is written where it lives (the env's -- or the pool entry's -- table in global memory: worldgen only
// ever appends to it) and no night-frame pixel buffer is kept (a reset frame is step 0: day).  73 -> 29 KB per workgroup:
// the regeneration kernel, launched after EVERY step to look at an all but always empty queue, waited 100-340 us per step for
// a CU with 73 KB of LDS free next to the generation kernels at 8192 x 256x256 (r4f / r4g).
__host__ __device__ inline LdsLayout big_reset_layout(const Config& c) {
  LdsLayout L = lds_layout(c);
  if (L.maps_in_lds) return L;
  int o = 0;
  L.frame = 0;
  L.frame_bytes = 0;
  L.frame_over_objs = 0;
  L.objs = -1;
  layout_tail(L, o, c, CRAFTER_RULES_HEAD_BYTES, true);
  L.wg = o; L.mtb = o + 1024; o += align16(WG_LDS_BYTES);
  layout_end(L, o, align16(render_lds_bytes(c)));
  return L;
}

// crafter_edit_envs (env_edit.hpp): the env's tables where big_reset_layout keeps them -- an LDS-resident world's maps and slot
// table staged, a large world's left where they live -- and nothing else: an edit neither generates nor draws, so no worldgen
// scratch, no pixel buffer and no renderer region.  20,352 B for the default geometry, 14,272 B for 256x256.
__host__ __device__ inline LdsLayout edit_layout(const Config& c) {
  LdsLayout L = lds_layout(c);   // (for maps_in_lds: the one decision every kernel over the same state shares)
  int cells = c.W * c.H;
  int o = 0;
  L.frame = 0;
  L.frame_bytes = 0;
  L.frame_over_objs = 0;
  L.wg = L.mtb = -1;
  if (L.maps_in_lds) {
    L.mat = o;        o += align16(cells);
    L.objmap = o;     o += align16(2 * cells);
    L.objs = o;       o += 16 * c.max_objects;
  } else {
    L.mat = L.objmap = -1;
    L.objs = -1;
  }
  layout_tail(L, o, c, CRAFTER_RULES_HEAD_BYTES, true);
  layout_end(L, o, 0);
  return L;
}

// LDS of the frame kernel: record | MT state | second MT state | frame record | night pixel buffer | renderer region
struct FrameLayout {
  int rec, mt, mtb, cells, pix, pix_bytes, scratch, render, total;
};
// (a night frame's pixel buffer is the env's scratch in global memory: frame_night_px_words per env)
__host__ __device__ inline int frame_night_px_words(const Config& c) { return align16(4 * c.local_gw * c.unit_x * c.local_gh * c.unit_y) / 4; }
__host__ __device__ inline FrameLayout frame_layout(const Config& c) {
  FrameLayout F;
  int o = 0;
  F.rec = o;    o += align16((int)sizeof(EnvRec));
  F.mt = o;     o += align16(4 * MT_N);
  F.mtb = o;    o += align16(4 * MT_N);
  F.cells = o;  o += kFrameRecordBytes;
  F.pix = o;    F.pix_bytes = 0;
  F.scratch = o; o += 16;
  F.render = o; o += align16(render_lds_bytes(c));
  F.total = o;
  return F;
}

constexpr int kGenSeedLds = ((4 * MT_N + 15) / 16 * 16) + 1024 + 16;   // mt | perm, pg3, source, ridx | scratch

// A world's cells are independent: `parts` workgroups share one world (part p classifies cells [p, p + 1) * cells / parts),
// so a batch of few worlds still spreads over the chip and finishes in a fraction of a world's serial time.
constexpr int kGenClassifyTables = 512 + kSimplexLdsBytes;   // perm, gradient numbers | noise3's tables (simplex.hpp)
constexpr int kGenClassifyCells = 1024;   // cells per workgroup (4 per thread): rounds of a few hundred look-ups keep the lanes busy
__host__ __device__ inline int gen_classify_parts(const Config& c) {
  return (c.W * c.H + kGenClassifyCells - 1) / kGenClassifyCells;
}

// LDS of the classification kernel: tables | state bytes | work list | counter (for `per` cells per workgroup)
__host__ __device__ inline int gen_classify_lds_bytes(const Config&) { return kGenClassifyTables + 3 * kGenClassifyCells + 16; }

struct GenResolveLayout {
  int mat, objs, mt, wg, rec, rules, chunk_order, chunk_seen, census, scratch, total;
};
__host__ __device__ inline GenResolveLayout gen_resolve_layout(const Config& c) {
  GenResolveLayout G;
  int cells = c.W * c.H, nch = c.nchunk_x * c.nchunk_y;
  int o = 0;
  G.mat = lds_layout(c).maps_in_lds ? o : -1;
  if (G.mat >= 0) o += align16(cells);
  // large worlds: the slot table is written straight into the pool entry (worldgen only appends; 32 KB for 2048 slots would
  // make a ONE-wave workgroup hold 54 KB of LDS: three of them took a CU's LDS away from the step kernel, r4g)
  G.objs = G.mat >= 0 ? o : -1;
  if (G.objs >= 0) o += 16 * c.max_objects;
  G.mt = o;           o += align16(4 * MT_N);
  G.wg = o;           o += align16(WG_LDS_BYTES);
  G.rec = o;          o += align16((int)sizeof(EnvRec));
  G.rules = o;        o += CRAFTER_RULES_HEAD_BYTES;
  G.chunk_order = o;  o += align16(2 * nch);
  G.chunk_seen = o;   o += align16(nch);
  G.census = o;       o += align16(20 * nch);
  G.scratch = o;      o += 16;
  G.total = o;
  return G;
}

}  // namespace crafter
