"""What the nearby-query tests share (tests/test_nearby_host.py: the kernel body on the CPU and the mirror; tests/test_gpu_nearby.py:
the device; tools/make_nearby_golden.py: the recorder of the reference fixture): the recorded runs, their tapes and poked states,
the reader of the fixture, the order of the entity list restated from the header, and authored worlds with the rows they must give.
Default rules: classes 0 none, 1 water, 2 grass, 3 stone, 4 path, 5 sand, 6 tree, 7 lava, 8 coal, 9 iron, 10 diamond, 11 table,
12 furnace, 13 player, 14 cow, 15 zombie, 16 skeleton, 17 arrow, 18 plant."""
import pathlib

import numpy as np

from crafter_amd import tables

N_MATERIALS = 12
MATERIALS = list(tables.load_rules()['materials'])
OBJECT_NAMES = ['player', 'cow', 'zombie', 'skeleton', 'arrow', 'plant']
CLASSES = ['none'] + MATERIALS + OBJECT_NAMES
N_CLASSES = len(CLASSES)
PLAYER, COW, ZOMBIE, SKELETON, ARROW, PLANT = range(1, 7)
ALL_OBJECTS = 0x3F << (N_MATERIALS + 1)
NOT_PLAYER = ALL_OBJECTS & ~(1 << (N_MATERIALS + PLAYER))

# ------------------------------------------------------------------ the reference fixture
FIXTURE = pathlib.Path(__file__).resolve().parent / 'golden' / 'reference_runs' / 'nearby_ref.npz'
DISTANCES = (0, 1, 2, 4, 7, 63, 64, 200)
RUNS = [((64, 64), s) for s in (1, 2, 3, 4, 5, 6)] + [((42, 30), s) for s in (1, 2, 3, 4)]
STEPS, EVERY = 60, 5                     # reset, then every fifth of 60 random steps: 13 states a run
POKE_SEED = 4                            # the poked states: the reset state of this seed, the player's record moved (every poke cell
                                         # holds no object in both areas: the recorder asserts it)


def run_key(area, seed):
  return f'{area[0]}x{area[1]}/{seed}'


def tape(seed):
  return np.random.RandomState(1000 + seed).randint(0, 17, size=STEPS).astype(np.int32)


def poke_positions(area):
  """Where the poked states put the player: numpy windows that are empty (one or two cells from the west / north border), clipped
  at the far borders, and re-clipped (a start that stays negative after the wrap comes back to 0)."""
  W, H = area
  return [(0, 0), (1, 5), (2, 2), (W - 1, H - 1), (W - 2, 0)]


def numpy_axis(p, d, L):
  """One axis of `a[p - d: p + d + 1]` as numpy reads it -> (start, stop), empty if start >= stop.  Written from the header."""
  start = p - d
  if start < 0:
    start += L
  if start < 0:
    start = 0
  return start, min(p + d + 1, L)


def sort_rows(objects, px, py, n_materials=N_MATERIALS, sleeping=False):
  """Canonical object tuples (type, x, y, health, fx, fy, aux) -> the entity list's rows (class, dx, dy, health, facing code, aux) in
  the header's order: ascending dx^2 + dy^2, then dx, then dy."""
  rows = []
  for tp, x, y, health, fx, fy, aux in objects:
    face = 1 if fx < 0 else 2 if fx > 0 else 3 if fy < 0 else 4
    code = (5 if sleeping else face) if tp == PLAYER else face if tp == ARROW else int(aux > 300) if tp == PLANT else 0
    rows.append((n_materials + tp, x - px, y - py, health, code, max(-32768, min(32767, aux))))
  return sorted(rows, key=lambda r: (r[1] * r[1] + r[2] * r[2], r[1], r[2]))


def load_fixture():
  """-> {run key or '<W>x<H>/poke': dict(pos int [S, 2], count int [S, 1 + n_materials] (World.count by material id), mats int [S, D]
  (bit m: material m is in World.nearby(pos, d)[0]), sleeping bool [S], objects: [S][D] lists of canonical tuples sorted by (x, y))}."""
  z = np.load(FIXTURE)
  out = {}
  for key in sorted({k.rsplit('/', 1)[0] for k in z.files if '/' in k}):
    pos, count, mats, rows = z[f'{key}/pos'], z[f'{key}/count'], z[f'{key}/mats'], z[f'{key}/objs']
    objects = [[[] for _ in DISTANCES] for _ in range(len(pos))]
    for s, di, *tup in rows.tolist():
      objects[s][di].append(tuple(tup))
    out[key] = dict(pos=pos.astype(int), count=count.astype(int), mats=mats.astype(int), objects=objects, sleeping=z[f'{key}/sleeping'].astype(bool))
  assert list(z['distances']) == list(DISTANCES)
  return out


def expected(entry, s, di, area, n_materials=N_MATERIALS):
  """What the NUMPY-window query must give for recorded state s and distance index di -> (material set as bits, the six object
  counts by type, the sorted rows of every object class, the number of cells of the window)."""
  px, py = (int(v) for v in entry['pos'][s])
  objs = entry['objects'][s][di]
  by_type = [sum(1 for o in objs if o[0] == t) for t in range(1, 7)]
  (x0, x1), (y0, y1) = numpy_axis(px, DISTANCES[di], area[0]), numpy_axis(py, DISTANCES[di], area[1])
  cells = max(x1 - x0, 0) * max(y1 - y0, 0)
  return int(entry['mats'][s][di]), by_type, sort_rows(objs, px, py, n_materials, bool(entry['sleeping'][s])), cells


def poke_oracle(orc, pos):
  """The player's record of OracleEnv `orc` moved to `pos` (its slot id moves with it); the cell must hold no object."""
  assert orc.objmap[pos] == 0 or (orc.ox[1], orc.oy[1]) == tuple(pos)
  orc.objmap[orc.ox[1], orc.oy[1]] = 0
  orc.objmap[pos] = 1
  orc.ox[1], orc.oy[1] = pos


# ------------------------------------------------------------------ authored worlds
def authored(W, H):
  """-> a list of dict(name, mat [W, H] of material names, objects (the player first, WorldBank's tuples), distance, classes (a
  set as bits), k, rows: the entity rows the query must give (None: not pinned), n, counts: {class name: count} that must hold)."""
  assert W >= 24 and H >= 18
  out = []
  grass = lambda: np.full((W, H), 'grass', dtype=object)
  cx, cy = W // 2, H // 2
  cow = N_MATERIALS + COW

  # (a) ties in dx^2 + dy^2: eight cows at (+-2, +-1) and (+-1, +-2), all at distance^2 5 -- ascending dx, then ascending dy
  order = [(-2, -1), (-2, 1), (-1, -2), (-1, 2), (1, -2), (1, 2), (2, -1), (2, 1)]
  objects = [('player', cx, cy, 0, (0, 1))] + [('cow', cx + dx, cy + dy, 3) for dx, dy in reversed(order)]
  out.append(dict(name='a-ties', mat=grass(), objects=objects, distance=3, classes=NOT_PLAYER, k=16,
                  rows=[(cow, dx, dy, 3, 0, 0) for dx, dy in order], n=8, counts={'none': 49, 'grass': 49, 'cow': 8, 'player': 1}))
  # ... and four of them, one of each sign pattern, with a nearer and a farther cow around them; k = 5 cuts the list behind the tie
  objects = [('player', cx, cy, 0, (0, 1)), ('cow', cx + 3, cy, 5), ('cow', cx + 2, cy + 1, 3), ('cow', cx - 1, cy + 2, 3), ('cow', cx - 2, cy - 1, 3),
             ('cow', cx + 1, cy - 2, 3), ('cow', cx, cy + 1, 2)]
  out.append(dict(name='a-ties-cut', mat=grass(), objects=objects, distance=None, classes=1 << cow, k=5,
                  rows=[(cow, 0, 1, 2, 0, 0), (cow, -2, -1, 3, 0, 0), (cow, -1, 2, 3, 0, 0), (cow, 1, -2, 3, 0, 0), (cow, 2, 1, 3, 0, 0)], n=6,
                  counts={'none': W * H, 'grass': W * H, 'cow': 6}))

  # (b) the facing code: arrows in the four directions, a ripe and an unripe plant, a zombie (0)
  mat = grass()
  mat[cx - 4: cx + 5, cy] = 'path'
  objects = [('player', cx, cy, 0, (1, 0)), ('arrow', cx - 1, cy, 0, (-1, 0)), ('arrow', cx + 1, cy, 0, (1, 0)), ('arrow', cx - 2, cy, 0, (0, -1)),
             ('arrow', cx + 2, cy, 0, (0, 1)), ('plant', cx, cy - 3, 1, (0, 1), 301), ('plant', cx, cy + 3, 1, (0, 1), 300), ('zombie', cx, cy + 4, 5, (0, 1), 3)]
  a, p, z = N_MATERIALS + ARROW, N_MATERIALS + PLANT, N_MATERIALS + ZOMBIE
  out.append(dict(name='b-facing', mat=mat, objects=objects, distance=4, classes=NOT_PLAYER, k=8,
                  rows=[(a, -1, 0, 0, 1, 0), (a, 1, 0, 0, 2, 0), (a, -2, 0, 0, 3, 0), (a, 2, 0, 0, 4, 0), (p, 0, -3, 1, 1, 301), (p, 0, 3, 1, 0, 300),
                        (z, 0, 4, 5, 0, 3)], n=7, counts={'none': 81, 'path': 9, 'grass': 72, 'arrow': 4, 'plant': 2, 'zombie': 1, 'player': 1}))

  # (c) aux beyond int16 on both sides
  objects = [('player', cx, cy, 0, (0, 1)), ('plant', cx + 1, cy, 1, (0, 1), 40000), ('zombie', cx - 1, cy, 5, (0, 1), -40000), ('plant', cx, cy + 2, 1, (0, 1), 32767)]
  out.append(dict(name='c-saturation', mat=grass(), objects=objects, distance=2, classes=NOT_PLAYER, k=4,
                  rows=[(z, -1, 0, 5, 0, -32768), (p, 1, 0, 1, 1, 32767), (p, 0, 2, 1, 1, 32767)], n=3, counts={'plant': 2, 'zombie': 1}))

  # (d) a class filter that excludes everything, and one that names the player alone
  objects = [('player', cx, cy, 0, (0, -1)), ('cow', cx + 1, cy, 3), ('zombie', cx, cy + 1, 5)]
  out.append(dict(name='d-no-class', mat=grass(), objects=objects, distance=5, classes=0, k=8, rows=[], n=0, counts={'cow': 1, 'zombie': 1, 'player': 1}))
  out.append(dict(name='d-skeletons-none', mat=grass(), objects=objects, distance=5, classes=1 << (N_MATERIALS + SKELETON), k=8, rows=[], n=0,
                  counts={'skeleton': 0}))
  out.append(dict(name='d-player', mat=grass(), objects=objects, distance=0, classes=1 << (N_MATERIALS + PLAYER), k=2,
                  rows=[(N_MATERIALS + PLAYER, 0, 0, 9, 3, 0)], n=1, counts={'none': 1, 'grass': 1, 'player': 1, 'cow': 0}))

  # (e) the player in each corner, a table diagonally inside and a cow two cells along each axis
  for name, (px, py) in dict(nw=(0, 0), ne=(W - 1, 0), sw=(0, H - 1), se=(W - 1, H - 1)).items():
    sx, sy = (1 if px == 0 else -1), (1 if py == 0 else -1)
    mat = grass()
    mat[px + sx, py + sy] = 'table'
    objects = [('player', px, py, 0, (sx, 0)), ('cow', px + 2 * sx, py, 3), ('cow', px, py + 2 * sy, 3)]
    rows = sorted([(cow, 2 * sx, 0, 3, 0, 0), (cow, 0, 2 * sy, 3, 0, 0)], key=lambda r: (r[1], r[2]))
    out.append(dict(name=f'e-corner-{name}', mat=mat, objects=objects, distance=2, classes=NOT_PLAYER, k=4, rows=rows, n=2,
                    counts={'none': 9, 'table': 1, 'grass': 8, 'cow': 2, 'player': 1}))
  return out
