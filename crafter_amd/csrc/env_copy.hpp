// Copies of whole environments between rows: crafter_copy_envs (row -> row of the bound state), crafter_save_envs (bound
// state -> a store) and crafter_load_envs (store -> bound state).  What an env IS (the state a deepcopy of the reference's
// crafter.Env carries) and what is derived or scratch is tabulated in DESIGN.md 3; the host builds a CopyPlan from that
// table (make_copy_plan) and the kernel only moves bytes.
#pragma once

#include <stdint.h>

#include "types.hpp"

namespace crafter {

constexpr int kCopyThreads = 256;
constexpr int kCheckThreads = 1024;
constexpr int kMaxCopySegs = 32;
constexpr long long kCopyBytesPerPart = 64 << 10;   // one workgroup per 64 KB of a pair: a 256x256 pair still spreads over the chip

enum : int { COPY_WITHIN = 0, COPY_SAVE = 1, COPY_LOAD = 2 };

// One per-env buffer: row r of the source starts at src + r * sstride, row r of the destination at dst + r * dstride.
// `bytes` are copied, the destination's bytes [bytes, dbytes) are zeroed (a store with a narrower slot table); src == null:
// the whole destination row is zeroed.  `width` (16, 4 or 1) is the widest access every row of both sides allows.
struct CopySeg {
  const uint8_t* src;
  uint8_t* dst;
  long long sstride, dstride;
  int bytes, dbytes, width, pad;
};

struct CopyPlan {
  CopySeg seg[kMaxCopySegs];
  int nseg;
  int parts;                    // workgroups per pair
  const EnvRec* episode_src;    // COPY_LOAD: gen_latest[dst] = episode_src[src].episode (the store holds no pool rows)
  int32_t* gen_latest;
};

__host__ inline bool plan_add(CopyPlan& p, const void* src, void* dst, long long sstride, long long dstride, int bytes, int dbytes) {
  if (!dst || p.nseg >= kMaxCopySegs) return dst == nullptr;
  CopySeg& s = p.seg[p.nseg++];
  s.src = (const uint8_t*)src;
  s.dst = (uint8_t*)dst;
  s.sstride = sstride;
  s.dstride = dstride;
  s.bytes = src ? bytes : 0;
  s.dbytes = dbytes;
  uintptr_t bits = (uintptr_t)src | (uintptr_t)dst | (uintptr_t)sstride | (uintptr_t)dstride | (uintptr_t)s.bytes | (uintptr_t)dbytes;
  s.width = (bits & 15) == 0 ? 16 : (bits & 3) == 0 ? 4 : 1;
  s.pad = 0;
  return true;
}

// One side of a copy: a state-pointer set (the bound state or a store), its rows and its slot-table width.
struct CopySide {
  const StatePtrs* st;
  int rows;
  int max_objects;
  const uint8_t* obs;
  const float* reward;
  const uint8_t* done;
};

// The rows of the DESIGN.md 3 table.  cfg: the bound state's configuration (both sides share its geometry).  pool_rows: both
// sides are the bound state and its pool is at rest (crafter_copy_envs).
// objmap_state: the cell -> slot map is state (maps in HBM, crafter_slot_map_derived() == 0); for LDS-resident worlds it
// is rebuilt from the slot table at every stage-in and never read.  Returns false if the plan does not fit.
__host__ inline bool make_copy_plan(CopyPlan& p, const Config& cfg, const CopySide& a, const CopySide& b, int mode,
                                    bool objmap_state, size_t obs_row, bool pool_rows) {
  p = CopyPlan{};
  const StatePtrs& s = *a.st;
  const StatePtrs& d = *b.st;
  const long long cells = (long long)cfg.W * cfg.H, nch = (long long)cfg.nchunk_x * cfg.nchunk_y;
  bool ok = true;
  auto row = [&](const void* src, void* dst, long long bytes) { ok = ok && plan_add(p, src, dst, bytes, bytes, (int)bytes, (int)bytes); };
  row(s.mat, d.mat, cells);
  if (objmap_state) row(s.objmap, d.objmap, cells * 2);
  ok = ok && plan_add(p, s.objs, d.objs, (long long)a.max_objects * sizeof(Obj), (long long)b.max_objects * sizeof(Obj),
                      a.max_objects * (int)sizeof(Obj), b.max_objects * (int)sizeof(Obj));
  row(s.mt, d.mt, MT_N * 4);
  row(s.rec, d.rec, sizeof(EnvRec));
  row(s.chunk_order, d.chunk_order, nch * 2);
  row(s.chunk_seen, d.chunk_seen, nch);
  row(s.census, d.census, nch * 5 * 4);
  if (s.terminal && d.terminal) row(s.terminal, d.terminal, (MAX_ACH + 4) * 4);
  if (s.semantic && d.semantic) row(s.semantic, d.semantic, cells);
  if (a.obs && b.obs) row(a.obs, (void*)b.obs, (long long)obs_row);
  if (a.reward && b.reward) row(a.reward, (void*)b.reward, 4);
  if (a.done && b.done) row(a.done, (void*)b.done, 1);
  if (mode == COPY_WITHIN && pool_rows) {
    // both sides are the live state of one batch: the source's two pooled worlds (at rest: see crafter_copy_envs) go along
    const long long n = cfg.num_envs, C = cfg.max_objects;
    for (int e = 0; e < 2; e++) {
      row(s.pool_mat + e * n * cells, d.pool_mat + e * n * cells, cells);
      row(s.pool_objs + e * n * C, d.pool_objs + e * n * C, C * sizeof(Obj));
      row(s.pool_mt + e * n * MT_N, d.pool_mt + e * n * MT_N, MT_N * 4);
      row(s.pool_hdr + e * n, d.pool_hdr + e * n, sizeof(PoolHdr));
      row(s.pool_chunk_order + e * n * nch, d.pool_chunk_order + e * n * nch, nch * 2);
      row(s.pool_perm + e * n * 512, d.pool_perm + e * n * 512, 512);
      row(s.pool_census + e * n * nch * 5, d.pool_census + e * n * nch * 5, nch * 5 * 4);
    }
    row(s.gen_latest, d.gen_latest, 4);
  } else if (mode != COPY_SAVE && d.pool_hdr) {
    // a store has no pool rows (nor has a pool that failed: its entries may still be written): the destination's entries are
    // emptied (ready = 0, pending = 0), it regenerates its next world inline once and asks the pool again from there
    // (gen_latest = the loaded episode)
    const long long n = cfg.num_envs;
    for (int e = 0; e < 2; e++) ok = ok && plan_add(p, nullptr, d.pool_hdr + e * n, 0, sizeof(PoolHdr), 0, sizeof(PoolHdr));
    p.episode_src = s.rec;
    p.gen_latest = d.gen_latest;
  }
  long long bytes = 0;
  for (int i = 0; i < p.nseg; i++) bytes += p.seg[i].dbytes;
  p.parts = (int)((bytes + kCopyBytesPerPart - 1) / kCopyBytesPerPart);
  if (p.parts < 1) p.parts = 1;
  return ok;
}

template <class T>
__device__ __forceinline__ void copy_units(const CopySeg& g, const uint8_t* src, uint8_t* dst, int first, int step) {
  const int n = g.bytes / (int)sizeof(T), nd = g.dbytes / (int)sizeof(T);
  const T* s = (const T*)src;
  T* d = (T*)dst;
  for (int i = first; i < n; i += step) d[i] = s[i];
  if (nd > n) {
    T z;
    __builtin_memset(&z, 0, sizeof(T));
    for (int i = n + (first - n % step + step) % step; i < nd; i += step) d[i] = z;
  }
}

// Validates the indices of one call before anything is copied (one workgroup; no host read-back): every index in range, no
// destination row named twice, and for a copy within the batch no destination that is also a source.  mark[]: one word per
// row of the bound state, stamped with this call's number (no clearing between calls).  A refused call sets *verdict and
// ST_BAD_COPY in the status of every bound-state row it names that exists (row 0 if none does); the copy kernel behind it
// then moves nothing.
__global__ void __launch_bounds__(kCheckThreads)
crafter_copy_check_kernel(const int32_t* __restrict__ sidx, const int32_t* __restrict__ didx, int n, int src_rows, int dst_rows,
                          int mode, int32_t stamp, int32_t* __restrict__ mark, int32_t* __restrict__ verdict, EnvRec* __restrict__ rec,
                          int rows) {
  __shared__ int bad, named;
  if (threadIdx.x == 0) bad = named = 0;
  __syncthreads();
  const bool mark_dst = mode != COPY_SAVE;
  for (int i = (int)threadIdx.x; i < n; i += kCheckThreads) {
    int s = sidx ? sidx[i] : i, d = didx ? didx[i] : i;
    if (s < 0 || s >= src_rows || d < 0 || d >= dst_rows) {
      bad = 1;
    } else if (mark_dst) {
      if (atomicExch(mark + d, stamp) == stamp) bad = 1;   // the second claim of a destination row
    }
  }
  __syncthreads();
  if (mode == COPY_WITHIN)
    for (int i = (int)threadIdx.x; i < n; i += kCheckThreads) {
      int s = sidx[i];
      if (s >= 0 && s < src_rows && __hip_atomic_load(mark + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == stamp) bad = 1;
    }
  __syncthreads();
  if (bad) {
    for (int i = (int)threadIdx.x; i < n; i += kCheckThreads) {
      int r = mode == COPY_SAVE ? (sidx ? sidx[i] : i) : (didx ? didx[i] : i);
      if (r >= 0 && r < rows) {
        atomicOr(&rec[r].status, (uint32_t)ST_BAD_COPY);
        named = 1;
      }
    }
    __syncthreads();
    if (threadIdx.x == 0 && !named) atomicOr(&rec[0].status, (uint32_t)ST_BAD_COPY);
  }
  if (threadIdx.x == 0) *verdict = bad;
}

// Pair blockIdx.x / parts, part blockIdx.x % parts: each of the plan's rows is split over the pair's workgroups.
__global__ void __launch_bounds__(kCopyThreads)
crafter_copy_envs_kernel(CopyPlan plan, const int32_t* __restrict__ sidx, const int32_t* __restrict__ didx, int n,
                         const int32_t* __restrict__ verdict) {
  if (*verdict) return;
  const int pair = (int)blockIdx.x / plan.parts, part = (int)blockIdx.x % plan.parts;
  if (pair >= n) return;
  const long long s = sidx ? sidx[pair] : pair, d = didx ? didx[pair] : pair;
  const int first = part * kCopyThreads + (int)threadIdx.x, step = plan.parts * kCopyThreads;
  for (int k = 0; k < plan.nseg; k++) {
    const CopySeg& g = plan.seg[k];
    const uint8_t* src = g.src + s * g.sstride;
    uint8_t* dst = g.dst + d * g.dstride;
    if (g.width == 16) copy_units<uint4>(g, src, dst, first, step);
    else if (g.width == 4) copy_units<uint32_t>(g, src, dst, first, step);
    else copy_units<uint8_t>(g, src, dst, first, step);
  }
  if (plan.gen_latest && part == 0 && threadIdx.x == 0) plan.gen_latest[d] = plan.episode_src[s].episode;
}

}  // namespace crafter
