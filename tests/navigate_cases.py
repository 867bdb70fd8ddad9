"""Authored worlds for the navigation query, with the values they must give, shared by tests/test_navigate_host.py (the kernel
bodies on the CPU) and tests/test_gpu_navigate.py (the device).  Default rules: classes 0 none, 1 water, 2 grass, 3 stone,
4 path, 5 sand, 6 tree, 7 lava, 8 coal, 9 iron, 10 diamond, 11 table, 12 furnace, 13 player, 14 cow ... 18 plant; actions 1 .. 4
move left, right, up, down."""
import numpy as np

from crafter_amd import tables

LEFT, RIGHT, UP, DOWN = 1, 2, 3, 4
MOVES = [LEFT, RIGHT, UP, DOWN]
N_MATERIALS = 12
CLASSES = ['none'] + list(tables.load_rules()['materials']) + ['player', 'cow', 'zombie', 'skeleton', 'arrow', 'plant']
WALKABLE = ['grass', 'path', 'sand']
# sixteen entries: single materials, two sets, every object class -- `player` is -1 everywhere (its own cell does not count)
TARGETS16 = ['water', 'grass', 'stone', 'path', 'sand', 'tree', 'lava', ['coal', 'iron', 'diamond'], 'table', 'cow', 'zombie', 'skeleton',
             'plant', 'player', 'arrow', ['tree', 'cow']]


def class_set(entry):
  items = entry if isinstance(entry, (list, tuple)) else [entry]
  return sum(1 << (CLASSES.index(i) if isinstance(i, str) else int(i)) for i in items)


def sets(targets):
  return [class_set(t) for t in targets]


def _world(W, H, fill):
  return np.full((W, H), fill, dtype=object)


def cases(W, H):
  """-> a list of dict(name, mat [W, H] of material names, objects (the player first), targets, passable (None: the default),
  expect: per target (dist, first, facing))."""
  assert W >= 24 and H >= 18
  out = []

  # (a) a serpentine corridor over the whole map, one cell wide: down column 0, over at the bottom, up column 2, ...
  mat = _world(W, H, 'stone')
  cols = list(range(0, W, 2))
  path = []
  for k, x in enumerate(cols):
    ys = range(H) if k % 2 == 0 else range(H - 1, -1, -1)
    path += [(x, y) for y in ys]
    if k + 1 < len(cols):
      path.append((x + 1, path[-1][1]))
  for x, y in path:
    mat[x, y] = 'grass'
  mat[path[-1]] = 'table'
  out.append(dict(name='a-serpentine', mat=mat, objects=[('player', 0, 0, 0, (0, 1))], targets=['table', 'tree'], passable=None,
                  expect=[(len(path) - 1, DOWN, 0), (-1, -1, 0)]))
  assert len(path) - 1 == len(cols) * H + len(cols) - 2

  # (b) a target walled in by water; the water itself is reached in a straight walk
  mat = _world(W, H, 'grass')
  mat[4:7, 4:7] = 'water'
  mat[5, 5] = 'diamond'
  px, py = W // 2, H // 2
  out.append(dict(name='b-walled-in', mat=mat, objects=[('player', px, py, 0, (0, 1))], targets=['diamond', 'water'], passable=None,
                  expect=[(-1, -1, 0), (px - 6 + py - 6, LEFT, 0)]))

  # (c) two equally near targets left and up, then right and down: left, right, up, down is the order
  mat = _world(W, H, 'grass')
  mat[7, 10] = mat[10, 7] = 'tree'
  mat[13, 10] = mat[10, 13] = 'coal'
  mat[10, 15] = mat[10, 5] = 'iron'
  out.append(dict(name='c-ties', mat=mat, objects=[('player', 10, 10, 0, (0, 1))], targets=['tree', 'coal', ['tree', 'coal']], passable=None,
                  expect=[(3, LEFT, 0), (3, RIGHT, 0), (3, LEFT, 0)]))

  # (d) a cow in a one-wide corridor: no way past it; with a bypass, the detour.  The cow as the target: up to the cow
  for bypass in (False, True):
    mat = _world(W, H, 'stone')
    mat[2:21, 10] = 'grass'
    mat[21, 10] = 'table'
    if bypass:
      mat[9:12, 11] = 'grass'
    out.append(dict(name=f'd-cow-{"bypass" if bypass else "blocked"}', mat=mat, objects=[('player', 2, 10, 0, (1, 0)), ('cow', 10, 10)],
                    targets=['table', 'cow'], passable=None, expect=[(21 if bypass else -1, RIGHT if bypass else -1, 0), (8, RIGHT, 0)]))

  # (e) the player in every corner and on every edge, the targets on the opposite borders: nothing wraps around
  for px, py in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2, H - 1), (0, H // 2), (W - 1, H // 2)):
    mat = _world(W, H, 'grass')
    tx = 0 if px == W - 1 else W - 1
    ty = 0 if py == H - 1 else H - 1
    mat[tx, py] = 'tree'
    mat[px, ty] = 'coal'
    facing_coal = 1 if (py + 1 == ty) else 0   # (never: H >= 18)
    out.append(dict(name=f'e-border-{px}-{py}', mat=mat, objects=[('player', px, py, 0, (0, 1))], targets=['tree', 'coal'], passable=None,
                    expect=[(abs(tx - px), RIGHT if tx > px else LEFT, 0), (abs(ty - py), DOWN if ty > py else UP, facing_coal)]))

  # (f) adjacent and faced; adjacent, not faced
  mat = _world(W, H, 'grass')
  mat[11, 10] = 'tree'
  mat[10, 9] = 'coal'
  out.append(dict(name='f-adjacent', mat=mat, objects=[('player', 10, 10, 0, (1, 0))], targets=['tree', 'coal'], passable=None,
                  expect=[(1, RIGHT, 1), (1, UP, 0)]))

  # (g) a walkable target behind a strip of lava: walked around by default, crossed when lava is passable
  mat = _world(W, H, 'grass')
  mat[14, 5:16] = 'lava'
  mat[18, 10] = 'sand'
  for passable, d in ((None, 20), (WALKABLE + ['lava'], 8)):
    out.append(dict(name=f'g-lava-{"crossed" if passable else "around"}', mat=mat, objects=[('player', 10, 10, 0, (0, 1))], targets=['sand'],
                    passable=passable, expect=[(d, RIGHT, 0)]))
  return out


def woodcutter_worlds(W, H, n, seed=0):
  """n worlds of sand, stone, water and trees only, the player the only object: no grass and no path, so no creature can ever
  spawn (env.py:141-155) and the worlds are deterministic.  -> (mats, objects)."""
  rs = np.random.RandomState(seed)
  mats, objects = [], []
  for _ in range(n):
    mat = _world(W, H, 'sand')
    r = rs.rand(W, H)
    mat[r < 0.12] = 'stone'
    mat[(r >= 0.12) & (r < 0.20)] = 'water'
    mat[(r >= 0.20) & (r < 0.215)] = 'tree'
    px, py = W // 2, H // 2
    mat[px - 1:px + 2, py - 1:py + 2] = 'sand'
    mats.append(mat)
    objects.append([('player', px, py, 0, (0, 1))])
  return mats, objects
