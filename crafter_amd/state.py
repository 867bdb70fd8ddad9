"""Shapes and views of the per-env state buffers (crafter_hip_types.h crafter_state_ptrs), backend-agnostic.

The buffers themselves are allocated by the caller (torch tensors on the GPU in the product);
this module only says how big they are and how to read them back as structured numpy arrays.
"""
import numpy as np

from . import abi


def state_spec(cfg):
  """name -> (shape, numpy dtype) of every caller-owned state buffer."""
  n, cells = cfg.num_envs, cfg.W * cfg.H
  nch = cfg.nchunk_x * cfg.nchunk_y
  return {
      'mat': ((n, cells), np.uint8),
      'objmap': ((n, cells), np.uint16),
      'objs': ((n, cfg.max_objects, abi.OBJ_DTYPE.itemsize), np.uint8),
      'mt': ((n, abi.MT_N), np.uint32),
      'rec': ((n, abi.REC_DTYPE.itemsize), np.uint8),
      'chunk_order': ((n, nch), np.uint16),
      'chunk_seen': ((n, nch), np.uint8),
      'census': ((n, nch * 5), np.int32),
      'semantic': ((n, cells), np.uint8),
      'reset_q': ((2, n + 4), np.int32),
      # world pool (only allocated with auto_reset)
      'pool_mat': ((2, n, cells), np.uint8),
      'pool_objs': ((2, n, cfg.max_objects, abi.OBJ_DTYPE.itemsize), np.uint8),
      'pool_mt': ((2, n, abi.MT_N), np.uint32),
      'pool_hdr': ((2, n, abi.POOL_HDR_DTYPE.itemsize), np.uint8),
      'pool_chunk_order': ((2, n, nch), np.uint16),
      'gen_q': ((8, 4 * n + 4), np.int32),
      'gen_latest': ((n,), np.int32),
      'terminal': ((n, abi.MAX_ACH + 4), np.int32),
      'pool_stats': ((4,), np.int32),
      'pool_perm': ((2, n, 512), np.uint8),
      'pool_census': ((2, n, nch * 5), np.int32),
  }


# What a copy of an env carries: its state rows, without the world pool's buffers or the request queues.
STORE_BUFFERS = ('mat', 'objmap', 'objs', 'mt', 'rec', 'chunk_order', 'chunk_seen', 'census', 'terminal', 'semantic')


def store_spec(cfg, rows, slot_map_derived=True):
  """name -> (shape, numpy dtype) of the buffers an EnvStore of `rows` envs holds: the state rows (objmap only where the
  cell -> slot map is state, i.e. not slot_map_derived; semantic only with want_semantic) and the last obs / reward / done."""
  spec = state_spec(cfg)
  out = {}
  for name in STORE_BUFFERS:
    if (name == 'objmap' and slot_map_derived) or (name == 'semantic' and not cfg.want_semantic):
      continue
    shape, dt = spec[name]
    out[name] = ((rows,) + tuple(shape[1:]), dt)
  out['obs'] = ((rows, cfg.size_h, cfg.size_w, 3), np.uint8)
  out['reward'] = ((rows,), np.float32)
  out['done'] = ((rows,), np.uint8)
  return out


POOL_BUFFERS = ('pool_mat', 'pool_objs', 'pool_mt', 'pool_hdr', 'pool_chunk_order', 'gen_q', 'gen_latest', 'pool_stats', 'pool_perm', 'pool_census')


def seed_lanes(seeds):
  """CPython ``hash(seed)`` as the unsigned 64-bit lane of the tuple hash in env.py:74.
  Works for any hashable seed the reference would accept, not only ints."""
  return np.array([hash(s) & 0xFFFFFFFFFFFFFFFF for s in seeds], dtype=np.uint64)


MAX_LEVELS = 65536   # capacity of a handle's level table (include/crafter_hip.h crafter_set_levels)


def _u64(values):
  """Anything that holds 64 lane bits (uint64, int64 bit patterns, Python ints of either sign) -> uint64 array."""
  a = np.asarray(values)
  if a.dtype == np.uint64:
    return a
  if a.dtype.kind == 'i':
    return a.astype(np.int64).view(np.uint64)
  if a.dtype.kind == 'u':
    return a.astype(np.uint64)
  flat = [int(v) & 0xFFFFFFFFFFFFFFFF for v in np.asarray(values, dtype=object).reshape(-1)]
  return np.array(flat, dtype=np.uint64).reshape(np.shape(values))


GOLDEN64 = np.uint64(0x9E3779B97F4A7C15)


def mix64(z):
  """splitmix64's finaliser over a uint64 array (csrc/env_levels.hpp mix64), mod 2^64."""
  with np.errstate(over='ignore'):
    z = np.asarray(z, np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def levels_pick(lanes, k, K, cum=None, key=0):
  """The numpy mirror of the device's `pick` (include/crafter_hip.h crafter_set_levels): the index of the level-table entry an
  env of draw lane `lanes` plays in its k-th episode, under a table of K entries, cumulative weights `cum` (uint32 [K], None:
  uniform) and `key`.  lanes (uint64, or int64 / Python ints carrying the 64 bits) and k (ints >= 0) broadcast against each other
  -> int32 array of that shape.  Exact: the device computes the same integers."""
  K = int(K)
  if not 1 <= K <= MAX_LEVELS:
    raise ValueError(f'K must lie in 1 .. {MAX_LEVELS}')
  lanes, k = np.broadcast_arrays(_u64(lanes), np.asarray(k, dtype=np.int64).astype(np.uint64))
  with np.errstate(over='ignore'):
    u = mix64(lanes + GOLDEN64 * k + np.uint64(int(key) & 0xFFFFFFFFFFFFFFFF)) >> np.uint64(32)
    if cum is None:
      return ((u * np.uint64(K)) >> np.uint64(32)).astype(np.int32)
  cum = np.asarray(cum)
  if cum.shape != (K,):
    raise ValueError(f'cum must have shape ({K},)')
  # first j with cum[j] > u; cum[K - 1] counts as 2^32 whatever it holds
  return np.minimum(np.searchsorted(cum[:K - 1].astype(np.uint64), u, side='right'), K - 1).astype(np.int32)


def fingerprint_units(snapshot, seed_lane):
  """The canonical unit sequences a state fingerprint hashes (include/crafter_hip_fingerprint.h): a list of FP_PARTS
  uint64 arrays -- map, objects, player, clock, rng, chunks, ident -- from a snapshot() dict (BatchedEnv's or OracleEnv's) and
  the env's seed lane (seed_lanes)."""
  u32 = lambda values: (np.asarray(values, np.int64) & 0xFFFFFFFF).astype(np.uint64).reshape(-1)
  mat = np.ascontiguousarray(snapshot['mat'], np.uint8)
  H = mat.shape[1]
  cells = mat.reshape(-1)
  padded = np.zeros((cells.size + 7) // 8 * 8, np.uint8)
  padded[:cells.size] = cells
  objects = np.zeros((len(snapshot['objects']), 2), np.uint64)
  for k, (tp, x, y, health, fx, fy, aux) in enumerate(snapshot['objects']):
    objects[k, 0] = int(tp) | (int(health) & 0xFF) << 8 | (int(fx) & 0xFF) << 16 | (int(fy) & 0xFF) << 24 | int(x) << 32 | int(y) << 48
    objects[k, 1] = int(aux) & 0xFFFFFFFF
  player = list(snapshot['inventory']) + list(snapshot['achievements']) + [int(bool(snapshot['sleeping']))] + [
      snapshot[k] for k in ('hunger2', 'thirst2', 'fatigue2', 'recover2', 'player_last_health')]
  mt = np.asarray(snapshot['mt_key'], np.uint32).astype(np.uint64)
  nchunk_y = (H + abi.CHUNK - 1) // abi.CHUNK
  chunks = [xmin // abi.CHUNK * nchunk_y + ymin // abi.CHUNK for xmin, _, ymin, _ in snapshot['chunk_order']]
  return [padded.view('<u8').astype(np.uint64), objects.reshape(-1), u32(player), u32([snapshot['step']]),
          np.concatenate([mt[0::2] | mt[1::2] << np.uint64(32), u32([snapshot['mt_pos']])]), u32(chunks),
          np.concatenate([_u64([int(seed_lane)]), u32([snapshot['episode']])])]


def fingerprint_combine(part_hashes, parts):
  """K(parts) from the FP_PARTS part hashes of one env (a row of fingerprint_parts(), as ints of either sign) -> unsigned int."""
  parts = int(parts)
  if not 0 < parts <= abi.FP_ALL:
    raise ValueError(f'parts must be a non-empty mask of bits 0 .. {abi.FP_PARTS - 1}')
  total = sum(int(h) for p, h in enumerate(part_hashes) if parts >> p & 1) & 0xFFFFFFFFFFFFFFFF
  with np.errstate(over='ignore'):
    return int(mix64(np.uint64(parts) * GOLDEN64 + np.uint64(total)))


def fingerprint_host(snapshot, seed_lane, parts=abi.FP_ALL):
  """The numpy mirror of the device's state fingerprint (include/crafter_hip_fingerprint.h), from a snapshot() dict
  -- BatchedEnv.snapshot(i) or OracleEnv.snapshot() -- and the env's seed lane -> (key over the part mask `parts`, the
  FP_PARTS part hashes), unsigned Python ints.  Exact: the device computes the same integers."""
  hashes = []
  with np.errstate(over='ignore'):
    for p, units in enumerate(fingerprint_units(snapshot, seed_lane)):
      salt = mix64(np.uint64(p + 1))
      terms = mix64((units ^ salt) + np.arange(1, units.size + 1, dtype=np.uint64) * GOLDEN64)
      hashes.append(int(mix64(salt + np.uint64(units.size) + terms.sum(dtype=np.uint64))))
  return fingerprint_combine(hashes, parts), hashes


def navigate_host(snapshot, n_materials, targets, passable, move_actions):
  """The Python mirror of the device's navigation query (include/crafter_hip_navigate.h) over a snapshot() dict --
  BatchedEnv.snapshot(i) or OracleEnv.snapshot() -> (dist int32 [K], first int32 [K], facing bool [K]).  n_materials: the rules'
  material count (object class ids start behind it); targets: K class sets as ints (bit c = class c); passable: a set of
  material ids as an int; move_actions: the action indices of move left, right, up, down.  Written unlike the kernel on
  purpose: a queue-based breadth-first search that stores an integer distance per cell, then the rule for `first` over the
  four neighbours."""
  import collections
  mat = np.asarray(snapshot['mat'])
  W, H = mat.shape
  cls = mat.astype(np.int64).copy()
  free = np.zeros((W, H), bool)
  for m in range(1, n_materials + 1):
    if passable >> m & 1:
      free |= mat == m
  player = None
  for tp, x, y, _, fx, fy, _ in snapshot['objects']:
    cls[x, y] = n_materials + tp
    free[x, y] = False
    if tp == abi.T_PLAYER and player is None:
      player = (x, y, fx, fy)
  px, py, fx, fy = player
  free[px, py] = True
  steps = ((-1, 0), (1, 0), (0, -1), (0, 1))
  inside = lambda x, y: 0 <= x < W and 0 <= y < H
  K = len(targets)
  dist, first, facing = np.full(K, -1, np.int32), np.full(K, -1, np.int32), np.zeros(K, bool)
  for k, target in enumerate(targets):
    is_target = (int(target) >> cls & 1).astype(bool)
    is_target[px, py] = False
    d = np.full((W, H), -1, np.int64)
    queue = collections.deque()
    for x, y in zip(*np.nonzero(is_target)):
      d[x, y] = 0
      queue.append((int(x), int(y)))
    while queue:
      x, y = queue.popleft()
      for dx, dy in steps:
        nx, ny = x + dx, y + dy
        if inside(nx, ny) and d[nx, ny] < 0 and free[nx, ny]:   # (a target cell has its 0 already)
          d[nx, ny] = d[x, y] + 1
          queue.append((nx, ny))
    facing[k] = inside(px + fx, py + fy) and bool(is_target[px + fx, py + fy])
    if d[px, py] < 0:
      continue
    dist[k] = d[px, py]
    for a, (dx, dy) in zip(move_actions, steps):
      nx, ny = px + dx, py + dy
      if inside(nx, ny) and d[nx, ny] == d[px, py] - 1:   # (d >= 0: the cell is a target or free)
        first[k] = a
        break
  return dist, first, facing


def nearby_host(snapshot, n_materials, distance=None, k=16, classes=None, numpy_slices=False):
  """The numpy mirror of the device's nearby query (include/crafter_hip_nearby.h) over a snapshot() dict -- BatchedEnv.snapshot(i),
  OracleEnv.snapshot() or a CPU harness's -> (counts int32 [1 + n_materials + 6], ents int16 [k, 6], n).  distance: None or
  negative for the whole world; classes: a class set as an int (bit c = class c; None: every object class but the player);
  numpy_slices: the window is what the reference's own expression selects (engine.py:97-98), evaluated here by numpy itself.
  Written unlike the kernel on purpose: a boolean window, a bincount, a sort of tuples."""
  mat = np.asarray(snapshot['mat'])
  W, H = mat.shape
  nm, k = int(n_materials), int(k)
  if not 0 <= k <= abi.NEARBY_MAX_ENTS:
    raise ValueError(f'k must lie in 0 .. {abi.NEARBY_MAX_ENTS}')
  objects = 0x3F << (nm + 1)
  classes = objects & ~(1 << (nm + abi.T_PLAYER)) if classes is None else int(classes)
  if classes & ~objects:
    raise ValueError('classes names a class that is no object class')
  d = -1 if distance is None else int(distance)
  if numpy_slices and d < 0:
    raise ValueError('numpy_slices takes a distance >= 0')
  counts, ents = np.zeros(nm + 1 + abi.T_PLANT, np.int32), np.zeros((k, abi.NEARBY_ROW), np.int16)
  player = next((o for o in snapshot['objects'] if o[0] == abi.T_PLAYER), None)
  if not snapshot.get('episode', 1) or player is None:
    return counts, ents, 0
  px, py = int(player[1]), int(player[2])
  window = np.zeros((W, H), bool)
  if numpy_slices:
    window[px - d: px + d + 1, py - d: py + d + 1] = True
  elif d < 0:
    window[:] = True
  else:
    window[max(px - d, 0): px + d + 1, max(py - d, 0): py + d + 1] = True
  counts[0] = window.sum()
  counts[1: nm + 1] = np.bincount(mat[window].astype(np.int64), minlength=nm + 1)[1: nm + 1]
  rows = []
  for tp, x, y, health, fx, fy, aux in snapshot['objects']:
    if not window[x, y]:
      continue
    counts[nm + tp] += 1
    if classes >> (nm + tp) & 1:
      face = 1 if fx < 0 else 2 if fx > 0 else 3 if fy < 0 else 4
      code = ((5 if snapshot['sleeping'] else face) if tp == abi.T_PLAYER else face if tp == abi.T_ARROW else
              int(aux > 300) if tp == abi.T_PLANT else 0)
      dx, dy = x - px, y - py
      rows.append((dx * dx + dy * dy, dx, dy, nm + tp, health, code, min(max(int(aux), -32768), 32767)))
  rows.sort()
  for j, (_, dx, dy, cls, health, code, aux) in enumerate(rows[:k]):
    ents[j] = (cls, dx, dy, health, code, aux)
  return counts, ents, len(rows)


def _host_array(a, dtype):
  """A raw buffer -- numpy array or torch tensor, on any device -- as a contiguous numpy array viewed as `dtype`."""
  if hasattr(a, 'detach'):
    a = a.detach().cpu().numpy()
  a = np.ascontiguousarray(a)
  return a if a.dtype == dtype else a.view(dtype)


def audit_host(buffers, cfg, rules, slot_map_derived=True, mask=None):
  """The numpy mirror of the device's audit (include/crafter_hip_audit.h) over raw buffers -- a downloaded BatchedEnv.state or a
  CPU harness's buffers: mat, objs, rec, chunk_order, chunk_seen, census, and objmap unless slot_map_derived -> (flags int32 [N],
  detail int32 [N, 4]), rows with a zero mask byte left at 0 / -1.  cfg: the batch's abi.Config; rules: its compiled rules
  (n_materials, mat_grass, mat_path).  Written unlike the kernel on purpose -- per env, whole-array numpy, no shared counters --
  and exact: the device computes the same integers, `detail` included."""
  n, Wd, H, C = int(cfg.num_envs), int(cfg.W), int(cfg.H), int(cfg.max_objects)
  cells, ncy = Wd * H, int(cfg.nchunk_y)
  nch = int(cfg.nchunk_x) * ncy
  mat_all = _host_array(buffers['mat'], np.uint8).reshape(n, cells)
  objs_all = objs_view(_host_array(buffers['objs'], np.uint8).reshape(n, C, abi.OBJ_DTYPE.itemsize))
  rec_all = rec_view(_host_array(buffers['rec'], np.uint8).reshape(n, abi.REC_DTYPE.itemsize))
  order_all = _host_array(buffers['chunk_order'], np.uint16).reshape(n, nch)
  seen_all = _host_array(buffers['chunk_seen'], np.uint8).reshape(n, nch)
  census_all = _host_array(buffers['census'], np.int32).reshape(n, nch * 5)
  objmap_all = None if slot_map_derived else _host_array(buffers['objmap'], np.uint16).reshape(n, cells)
  cell_chunk = (np.arange(Wd)[:, None] // abi.CHUNK * ncy + np.arange(H)[None, :] // abi.CHUNK).reshape(-1)
  flags, detail = np.zeros(n, np.int32), np.full((n, 4), -1, np.int32)
  clamp = lambda v, lo, hi: min(max(int(v), lo), hi)
  for e in range(n):
    if mask is not None and not mask[e]:
      continue
    r = rec_all[e]
    if r['episode'] == 0:
      flags[e], detail[e] = abi.AUDIT_NOT_RESET, (0, -1, -1, -1)
      continue
    found = {}   # bit -> (index, found, expected) at the check's lowest offending index
    ranges = ((r['nobj'], 1, C), (r['mt_pos'], 0, abi.MT_N), (r['step'], 0, int(cfg.n_daylight) - 1), (r['nchunks_seen'], 0, nch))
    for field, (v, lo, hi) in enumerate(ranges):
      if not lo <= v <= hi:
        found[1] = (field, int(v), clamp(v, lo, hi))
        break
    nobj, k = clamp(r['nobj'], 1, C), clamp(r['nchunks_seen'], 0, nch)
    mat, objs, order = mat_all[e], objs_all[e], order_all[e][:k].astype(np.int64)
    # the chunk list
    pos = np.full(nch, -1, np.int64)
    for i in range(k - 1, -1, -1):
      if order[i] < nch:
        pos[order[i]] = i
    bad_pos = [i for i in range(k) if order[i] >= nch or pos[order[i]] != i]
    flagged = seen_all[e] != 0
    bad_pos += [int(pos[c]) for c in np.nonzero((pos >= 0) & ~flagged)[0]]
    unlisted = np.nonzero((pos < 0) & flagged)[0]
    if bad_pos:
      i = min(bad_pos)
      listed_once = order[i] < nch and pos[order[i]] == i
      found[9] = (i, 0, 1) if listed_once else (i, int(order[i]), -1)
    elif len(unlisted):
      found[9] = (-1, int(unlisted[0]), -1)
    # the slot table
    slots = np.arange(1, nobj)
    live = slots[objs['type'][1:nobj] != abi.T_NONE]
    lo = objs[live]
    players = (lo['type'] == abi.T_PLAYER) != (live == 1)
    bad_player = ([1] if nobj < 2 or objs['type'][1] == abi.T_NONE else []) + live[players].tolist()
    if bad_player:
      s = min(bad_player)
      tp = int(objs['type'][s]) if s < nobj else 0
      found[2] = (s, tp, abi.T_PLAYER if s == 1 else -1)
    ok = (lo['type'] <= abi.T_PLANT) & (lo['x'] < Wd) & (lo['y'] < H)
    if not ok.all():
      s = int(live[~ok][0])
      o = objs[s]
      found[3] = ((s, int(o['type']), abi.T_PLANT) if o['type'] > abi.T_PLANT else (s, int(o['x']), Wd - 1) if o['x'] >= Wd else
                  (s, int(o['y']), H - 1))
    valid, vo = live[ok], lo[ok]
    vcell = vo['x'].astype(np.int64) * H + vo['y']
    per_cell = np.bincount(vcell, minlength=cells)
    shared = np.nonzero(per_cell > 1)[0]
    if len(shared):
      found[4] = (int(shared[0]), int(per_cell[shared[0]]), 1)
    if objmap_all is not None:
      objmap = objmap_all[e]
      wrong = objmap[vcell] != valid
      if wrong.any():
        c = int(vcell[wrong].min())
        found[5] = (c, int(objmap[c]), int(valid[wrong & (vcell == c)].min()))
      elif int((objmap != 0).sum()) != len(live):
        found[5] = (-1, int((objmap != 0).sum()), len(live))
    bad_mat = np.nonzero((mat < 1) | (mat > rules.n_materials))[0]
    if len(bad_mat):
      found[6] = (int(bad_mat[0]), int(mat[bad_mat[0]]), -1)
    # the census
    count = np.zeros((nch, 5), np.int64)
    in_range = (mat >= 1) & (mat <= rules.n_materials)
    count[:, 0] = np.bincount(cell_chunk[in_range & (mat == rules.mat_grass)], minlength=nch)
    count[:, 1] = np.bincount(cell_chunk[in_range & (mat == rules.mat_path)], minlength=nch)
    vchunk = cell_chunk[vcell]
    for col, tp in ((2, abi.T_ZOMBIE), (3, abi.T_SKELETON), (4, abi.T_COW)):
      count[:, col] = np.bincount(vchunk[vo['type'] == tp], minlength=nch)
    stale = np.nonzero(census_all[e] != count.reshape(-1))[0]
    for bit, cols in ((7, stale[stale % 5 < 2]), (8, stale[stale % 5 >= 2])):
      if len(cols):
        found[bit] = (int(cols[0]), int(census_all[e][cols[0]]), int(count.reshape(-1)[cols[0]]))
    missing = valid[pos[vchunk] < 0]
    if len(missing):
      s = int(missing[0])
      found[10] = (s, int(cell_chunk[int(objs['x'][s]) * H + int(objs['y'][s])]), -1)
    if found:
      low = min(found)
      flags[e], detail[e] = sum(1 << b for b in found), (low,) + found[low]
  return flags, detail


def levels_cum(weights):
  """K weights (non-negative, not all zero) -> cum uint32 [K], cum[j] = min(floor(2^32 * sum(w[:j + 1]) / sum(w)), 2^32 - 1),
  in exact rational arithmetic."""
  from fractions import Fraction
  w = np.asarray(weights).reshape(-1)
  if w.size == 0 or w.dtype.kind not in 'iuf' or not np.all(np.isfinite(w.astype(np.float64))):
    raise ValueError('weights must be finite numbers')
  if (w < 0).any() or not (w > 0).any():
    raise ValueError('weights must be non-negative and not all zero')
  vals = [int(v) for v in w] if w.dtype.kind in 'iu' else [Fraction(float(v)) for v in w]
  total, acc, out = sum(vals), 0, np.zeros(w.size, np.uint32)
  for j, v in enumerate(vals):
    acc += v
    out[j] = min(int(Fraction(acc * 2 ** 32, 1) / total) if not isinstance(acc, int) else (acc << 32) // total, 2 ** 32 - 1)
  return out


def rec_view(rec_bytes):
  """uint8 [N, sizeof(EnvRec)] -> structured array [N]."""
  a = np.ascontiguousarray(rec_bytes)
  return a.view(abi.REC_DTYPE).reshape(a.shape[0])


def objs_view(objs_bytes):
  """uint8 [N, C, 16] -> structured array [N, C]."""
  a = np.ascontiguousarray(objs_bytes)
  return a.view(abi.OBJ_DTYPE).reshape(a.shape[0], a.shape[1])


def live_objects(objs_row, nobj, health):
  """Objects of one env in slot order as (type, x, y, health, fx, fy, aux) tuples -- the same
  canonical form as oracle.crafter_oracle.OracleEnv.objects()."""
  out = []
  for s in range(1, int(nobj)):
    o = objs_row[s]
    if o['type'] == abi.T_NONE:
      continue
    h = int(health) if o['type'] == abi.T_PLAYER else int(o['health'])
    out.append((int(o['type']), int(o['x']), int(o['y']), h, int(o['fx']), int(o['fy']), int(o['aux'])))
  return out


def occupied_cells(objs_row, nobj, cfg):
  """bool [W][H]: cells holding an object (World._obj_map != 0, engine.py:32), from the slot table."""
  occ = np.zeros((cfg.W, cfg.H), bool)
  for s in range(1, int(nobj)):
    o = objs_row[s]
    if o['type'] != abi.T_NONE:
      occ[int(o['x']), int(o['y'])] = True
  return occ


def chunk_keys(order_row, nseen, cfg):
  """chunk ids -> the reference's (xmin, xmax, ymin, ymax) keys (engine.py:112-117)."""
  keys = []
  for c in order_row[:int(nseen)]:
    cx, cy = divmod(int(c), cfg.nchunk_y)
    xmin, ymin = cx * abi.CHUNK, cy * abi.CHUNK
    keys.append((xmin, min(xmin + abi.CHUNK, cfg.W), ymin, min(ymin + abi.CHUNK, cfg.H)))
  return keys
