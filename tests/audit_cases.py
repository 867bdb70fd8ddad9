"""TEST INFRASTRUCTURE: the corruption table of the audit tests (CPU harness and GPU).  A case is applied to row i of a dict
of raw numpy buffers -- a CPU harness's `buf` or a downloaded BatchedEnv.state, the shapes of state.state_spec -- and returns what
the audit must say of that row: (the bits that must be set, bits that may be set as well, the detail row).  The expectations are
written from include/crafter_hip_audit.h, never from an audit's output.

A few cases need a record that no census column counts (a corrupt cow is, by the header's own rule, also a CREATURES finding):
`plant` authors one by hand, consistently, in the player's chunk."""
import numpy as np

from crafter_amd import abi, state

A = abi
BUFFERS = ('mat', 'objmap', 'objs', 'rec', 'chunk_order', 'chunk_seen', 'census')
_DTYPES = dict(mat=np.uint8, objmap=np.uint16, objs=np.uint8, rec=np.uint8, chunk_order=np.uint16, chunk_seen=np.uint8, census=np.int32)


class Ctx:
  """What a case needs beside the buffers: the geometry, the rules' ids, whether objmap is state."""

  def __init__(self, cfg, rules, map_state):
    self.cfg, self.rules, self.map_state = cfg, rules, bool(map_state)
    self.W, self.H, self.C = int(cfg.W), int(cfg.H), int(cfg.max_objects)
    self.ncy = int(cfg.nchunk_y)
    self.nch = int(cfg.nchunk_x) * self.ncy

  def chunk(self, x, y):
    return int(x) // A.CHUNK * self.ncy + int(y) // A.CHUNK


def host_buffers(tensors, ctx):
  """BatchedEnv.state (device tensors) -> private numpy copies of the buffers the audit reads, in state_spec's shapes."""
  return {k: state._host_array(tensors[k], _DTYPES[k]).copy() for k in BUFFERS if k != 'objmap' or ctx.map_state}


def row(b, i, ctx):
  """Writable views of row i: (rec record, objs [C], mat [W, H], objmap [W, H] or None, order [nch], seen [nch], census [nch, 5])."""
  rec = state.rec_view(b['rec'])
  objs = state.objs_view(b['objs'])
  assert np.shares_memory(rec, b['rec']) and np.shares_memory(objs, b['objs'])
  objmap = b['objmap'][i].reshape(ctx.W, ctx.H) if ctx.map_state else None
  return (rec[i:i + 1], objs[i], b['mat'][i].reshape(ctx.W, ctx.H), objmap, b['chunk_order'][i], b['chunk_seen'][i],
          b['census'][i].reshape(ctx.nch, 5))


def live_slots(b, i, ctx, types=None):
  rec, objs = row(b, i, ctx)[:2]
  return [s for s in range(1, int(rec['nobj'][0])) if objs[s]['type'] != A.T_NONE and (types is None or objs[s]['type'] in types)]


def occupied(b, i, ctx):
  objs = row(b, i, ctx)[1]
  return {(int(objs[s]['x']), int(objs[s]['y'])) for s in live_slots(b, i, ctx)}


def plant(b, i, ctx):
  """Adds a sapling to row i on a free grass cell of the player's chunk, every table following (it is no creature, its chunk is
  listed) -> its slot.  The row stays consistent."""
  rec, objs, mat, objmap, order, seen, census = row(b, i, ctx)
  n = int(rec['nobj'][0])
  assert n < ctx.C
  px, py = int(objs[1]['x']), int(objs[1]['y'])
  taken = occupied(b, i, ctx)
  cx, cy = px // A.CHUNK * A.CHUNK, py // A.CHUNK * A.CHUNK
  free = [(x, y) for x in range(cx, min(cx + A.CHUNK, ctx.W)) for y in range(cy, min(cy + A.CHUNK, ctx.H))
          if mat[x, y] == ctx.rules.mat_grass and (x, y) not in taken]
  assert free, 'no free grass cell in the player\'s chunk'
  x, y = free[0]
  objs[n] = np.zeros((), A.OBJ_DTYPE)
  objs[n]['type'], objs[n]['health'], objs[n]['x'], objs[n]['y'] = A.T_PLANT, 1, x, y
  rec['nobj'] = n + 1
  if objmap is not None:
    objmap[x, y] = n
  return n


# ---------------------------------------------------------------------------------------------- the cases
def _rec_case(field, index, value, expected, also=0, maybe=0):
  def case(b, i, ctx):
    rec, objs = row(b, i, ctx)[:2]
    if field == 'nobj':   # (records behind nobj are no state: cleared, so that a larger count brings nothing stale into the prefix)
      objs[int(rec['nobj'][0]):] = np.zeros((), A.OBJ_DTYPE)
    v, e = value(ctx), expected(ctx)
    rec[field] = v
    return A.AUDIT_REC | (also(ctx) if callable(also) else also), maybe, (1, index, v, e)
  return case


def _slot1_cow(b, i, ctx):
  objs = row(b, i, ctx)[1]
  objs[1]['type'] = A.T_COW
  return A.AUDIT_PLAYER | A.AUDIT_CREATURES, 0, (2, 1, A.T_COW, A.T_PLAYER)   # (a cow the census does not count)


def _second_player(b, i, ctx):
  s = plant(b, i, ctx)
  row(b, i, ctx)[1][s]['type'] = A.T_PLAYER
  return A.AUDIT_PLAYER, 0, (2, s, A.T_PLAYER, -1)


def _object_case(field, value, legal):
  def case(b, i, ctx):
    s = plant(b, i, ctx)
    v = value(ctx)
    row(b, i, ctx)[1][s][field] = v
    return A.AUDIT_OBJECT, 0, (3, s, v, legal(ctx))
  return case


def _shared_cell(b, i, ctx):
  s = plant(b, i, ctx)
  objs = row(b, i, ctx)[1]
  px, py = int(objs[1]['x']), int(objs[1]['y'])
  objs[s]['x'], objs[s]['y'] = px, py
  return A.AUDIT_CELL | (A.AUDIT_SLOTMAP if ctx.map_state else 0), 0, (4, px * ctx.H + py, 2, 1)


def _objmap_wrong_slot(b, i, ctx):
  s = plant(b, i, ctx)
  objs, _, objmap = row(b, i, ctx)[1:4]
  x, y = int(objs[s]['x']), int(objs[s]['y'])
  objmap[x, y] = 1
  return A.AUDIT_SLOTMAP, 0, (5, x * ctx.H + y, 1, s)


def _objmap_extra_cell(b, i, ctx):
  objmap = row(b, i, ctx)[3]
  x, y = np.argwhere(objmap == 0)[5]
  objmap[x, y] = 1
  n = len(live_slots(b, i, ctx))
  return A.AUDIT_SLOTMAP, 0, (5, -1, n + 1, n)


def _objmap_cleared_cell(b, i, ctx):
  s = plant(b, i, ctx)
  objs, _, objmap = row(b, i, ctx)[1:4]
  x, y = int(objs[s]['x']), int(objs[s]['y'])
  objmap[x, y] = 0
  return A.AUDIT_SLOTMAP, 0, (5, x * ctx.H + y, 0, s)


def _material_case(value):
  def case(b, i, ctx):
    mat = row(b, i, ctx)[2]
    R = ctx.rules
    x, y = np.argwhere((mat != R.mat_grass) & (mat != R.mat_path))[3]   # (a cell no census column counts)
    v = value(ctx)
    mat[x, y] = v
    return A.AUDIT_MATERIAL, 0, (6, int(x) * ctx.H + int(y), v, -1)
  return case


def _grass_to_sand(b, i, ctx):
  _, _, mat, _, _, _, census = row(b, i, ctx)
  x, y = np.argwhere(mat == ctx.rules.mat_grass)[7]
  mat[x, y] = ctx.rules.mat_sand
  c = ctx.chunk(x, y)
  return A.AUDIT_SPACE, 0, (7, c * 5, int(census[c, 0]), int(census[c, 0]) - 1)


def _zombie_freed(b, i, ctx):
  _, objs, _, _, _, _, census = row(b, i, ctx)
  zombies = live_slots(b, i, ctx, (A.T_ZOMBIE,))
  assert zombies, 'the row holds no zombie'
  s = zombies[0]
  c = ctx.chunk(objs[s]['x'], objs[s]['y'])
  n = len(live_slots(b, i, ctx))
  objs[s]['type'] = A.T_NONE
  if ctx.map_state:   # its cell still names the freed slot: one non-zero cell more than live records, and SLOTMAP is the lower bit
    return A.AUDIT_CREATURES | A.AUDIT_SLOTMAP, 0, (5, -1, n, n - 1)
  return A.AUDIT_CREATURES, 0, (8, c * 5 + 2, int(census[c, 2]), int(census[c, 2]) - 1)


def _cow_across_a_border(b, i, ctx):
  rec, objs, _, _, order, _, census = row(b, i, ctx)
  listed = set(order[:int(rec['nchunks_seen'][0])].tolist())
  taken = occupied(b, i, ctx)
  for s in live_slots(b, i, ctx, (A.T_COW,)):
    x, y = int(objs[s]['x']), int(objs[s]['y'])
    nx = x // A.CHUNK * A.CHUNK + A.CHUNK
    if nx >= ctx.W:
      nx = x // A.CHUNK * A.CHUNK - 1
    if nx < 0 or (nx, y) in taken or ctx.chunk(nx, y) not in listed:
      continue
    old, new = ctx.chunk(x, y), ctx.chunk(nx, y)
    objs[s]['x'] = nx
    word = min(old, new) * 5 + 4
    found = int(census[min(old, new), 4])
    if ctx.map_state:   # objmap names the slot where it stood, not where it stands: SLOTMAP is the lower bit
      return A.AUDIT_CREATURES | A.AUDIT_SLOTMAP, 0, (5, nx * ctx.H + y, 0, s)
    return A.AUDIT_CREATURES, 0, (8, word, found, found - 1 if old < new else found + 1)
  raise AssertionError('no cow beside a free cell of a listed neighbour chunk')


def _order_duplicate(b, i, ctx):
  rec, _, _, _, order = row(b, i, ctx)[:5]
  assert rec['nchunks_seen'][0] >= 2
  order[1] = order[0]
  return A.AUDIT_CHUNKS, A.AUDIT_CHUNK_MISSING, (9, 1, int(order[0]), -1)   # (an object may stand in the chunk that lost its entry)


def _order_out_of_range(b, i, ctx):
  order = row(b, i, ctx)[4]
  order[0] = ctx.nch
  return A.AUDIT_CHUNKS, A.AUDIT_CHUNK_MISSING, (9, 0, ctx.nch, -1)


def _flag_cleared(b, i, ctx):
  rec, _, _, _, order, seen = row(b, i, ctx)[:6]
  assert rec['nchunks_seen'][0] >= 3
  seen[order[2]] = 0
  return A.AUDIT_CHUNKS, 0, (9, 2, 0, 1)


def _flag_set(b, i, ctx):
  rec, _, _, _, order, seen = row(b, i, ctx)[:6]
  unlisted = sorted(set(range(ctx.nch)) - set(order[:int(rec['nchunks_seen'][0])].tolist()))
  assert unlisted, 'every chunk of the row is listed'
  seen[unlisted[-1]] = 1
  return A.AUDIT_CHUNKS, 0, (9, -1, unlisted[-1], -1)


def _list_shortened(b, i, ctx):
  rec, objs, _, _, order = row(b, i, ctx)[:5]
  k = int(rec['nchunks_seen'][0])
  homes = {ctx.chunk(objs[s]['x'], objs[s]['y']) for s in live_slots(b, i, ctx)}
  p = max(j for j in range(k) if int(order[j]) in homes)
  order[p], order[k - 1] = order[k - 1], order[p]   # (any order of the same chunks is a consistent row)
  rec['nchunks_seen'] = k - 1
  return A.AUDIT_CHUNKS | A.AUDIT_CHUNK_MISSING, 0, (9, -1, int(order[k - 1]), -1)


def _never_reset(b, i, ctx):
  rs = np.random.RandomState(77 + i)
  for k in b:
    raw = b[k][i].view(np.uint8)
    raw[...] = rs.randint(0, 256, size=raw.shape, dtype=np.uint8)
  state.rec_view(b['rec'])['episode'][i] = 0
  return A.AUDIT_NOT_RESET, 0, (0, -1, -1, -1)


_after_nobj_zero = lambda ctx: A.AUDIT_PLAYER | A.AUDIT_CREATURES | (A.AUDIT_SLOTMAP if ctx.map_state else 0)   # no record is left in the prefix
CASES = {
    'rec-nobj-high': _rec_case('nobj', 0, lambda c: c.C + 7, lambda c: c.C),
    'rec-nobj-zero': _rec_case('nobj', 0, lambda c: 0, lambda c: 1, also=_after_nobj_zero),
    'rec-mt-pos': _rec_case('mt_pos', 1, lambda c: 625, lambda c: 624),
    'rec-step': _rec_case('step', 2, lambda c: int(c.cfg.n_daylight), lambda c: int(c.cfg.n_daylight) - 1),
    # (the audit goes on with nch entries: what stands behind the list is read as part of it)
    'rec-nchunks': _rec_case('nchunks_seen', 3, lambda c: c.nch + 1, lambda c: c.nch, maybe=A.AUDIT_CHUNKS),
    'player-slot1-cow': _slot1_cow,
    'player-second': _second_player,
    'object-type': _object_case('type', lambda c: 200, lambda c: A.T_PLANT),
    'object-x': _object_case('x', lambda c: c.W, lambda c: c.W - 1),
    'object-y': _object_case('y', lambda c: 65535, lambda c: c.H - 1),
    'cell-shared': _shared_cell,
    'material-zero': _material_case(lambda c: 0),
    'material-high': _material_case(lambda c: int(c.rules.n_materials) + 1),
    'space-grass-to-sand': _grass_to_sand,
    'creatures-zombie-freed': _zombie_freed,
    'creatures-cow-across-a-border': _cow_across_a_border,
    'chunks-duplicate': _order_duplicate,
    'chunks-id-out-of-range': _order_out_of_range,
    'chunks-flag-cleared': _flag_cleared,
    'chunks-flag-set': _flag_set,
    'chunks-list-shortened': _list_shortened,
    'never-reset': _never_reset,
}
MAP_CASES = {   # only where objmap is state
    'slotmap-wrong-slot': _objmap_wrong_slot,
    'slotmap-extra-cell': _objmap_extra_cell,
    'slotmap-cleared-cell': _objmap_cleared_cell,
}


def cases(ctx):
  return dict(CASES, **MAP_CASES) if ctx.map_state else dict(CASES)


def corrupted(clean, name, rows, ctx):
  """-> (a copy of `clean` with case `name` applied to each of `rows`, {row: (bits, maybe, detail)})."""
  b = {k: v.copy() for k, v in clean.items()}
  return b, {i: cases(ctx)[name](b, i, ctx) for i in rows}


def check(flags, detail, want, where, untouched=()):
  """flags / detail of a batch against `want` ({row: (bits, maybe, detail)}): every other row must be 0 / -1, rows of `untouched`
  excepted."""
  for i in range(len(flags)):
    if i in untouched:
      continue
    bits, maybe, d = want.get(i, (0, 0, (-1, -1, -1, -1)))
    names = lambda v: [n for k, n in enumerate(A.AUDIT_NAMES) if v >> k & 1]
    assert int(flags[i]) & ~maybe == bits, f'{where} row {i}: flags {names(int(flags[i]))}, expected {names(bits)} (+ {names(maybe)})'
    assert tuple(int(v) for v in detail[i]) == tuple(d), f'{where} row {i}: detail {detail[i].tolist()}, expected {d}'
