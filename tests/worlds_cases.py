"""TEST INFRASTRUCTURE: the authored worlds, action tapes and oracle runs the authored-world tests share (CPU harness and GPU).
Every oracle run is computed once per session and never modified."""
import functools

import numpy as np

from crafter_amd import tables
from tests.worlds_ref import AuthoredOracle

RULES = tables.load_rules()
MAT = {n: i + 1 for i, n in enumerate(RULES['materials'])}
ACT = {n: i for i, n in enumerate(RULES['actions'])}
ITEMS = list(RULES['items'])
PLAYER, COW, ZOMBIE, SKELETON, ARROW, PLANT = range(1, 7)
T = 180   # daylight_of: night begins at step 148, so the last 30 frames are night frames with their noise draws


def inventory(**kw):
  return [int(kw.get(n, RULES['items'][n]['initial'])) for n in ITEMS]


def meadow(area=(64, 64)):
  """World 0: a meadow.  The player stands far from the centre, in another chunk, beside a table with wood in the inventory
  (make_wood_pickaxe is legal at once) and next to a zombie whose cooldown is 0 (it hits at step 1); four cows share each of
  six chunks (more than the balance pass tolerates: despawns) and at night the grass fills with zombies (spawns)."""
  W, H = area
  mat = np.full((W, H), MAT['grass'], np.uint8)
  mat[9, 11] = MAT['table']
  mat[20:24, 30] = MAT['tree']
  mat[0:3, 0:5] = MAT['water']
  objs = [(PLAYER, 10, 12, 0, (0, -1), 0), (ZOMBIE, 11, 12, 5, (0, 0), 0)]
  for cx, cy in [(1, 0), (2, 2), (0, 3), (3, 1), (1, 2), (2, 0)]:
    for k in range(4):
      objs.append((COW, 12 * cx + 2 + 2 * k, 12 * cy + 3 + k, 3, (0, 0), 0))
  return dict(mat=mat, objects=objs, inventory=inventory(wood=5, sapling=2, health=8))


def garden(area=(64, 64)):
  """World 1: the player at the centre (no PLAYER record) facing a ripe plant; an arrow in flight towards a stone wall, a
  second one towards a table (which it breaks); a young plant, water, sand and lava around."""
  W, H = area
  px, py = W // 2, H // 2
  mat = np.full((W, H), MAT['grass'], np.uint8)
  mat[px + 7, py - 8:py] = MAT['stone']
  mat[px - 6, py + 3] = MAT['table']
  mat[px - 10:px - 7, py - 3:py + 3] = MAT['water']
  mat[px + 3:px + 6, py + 5:py + 8] = MAT['sand']
  mat[px - 3, py + 9] = MAT['lava']
  mat[px + 1, py + 1] = MAT['furnace']
  objs = [(PLANT, px, py + 1, 1, (0, 0), 400), (ARROW, px + 2, py - 4, 0, (1, 0), 0), (ARROW, px - 2, py + 3, 0, (-1, 0), 0),
          (PLANT, px + 4, py + 2, 1, (0, 0), 7), (COW, px - 4, py - 5, 3, (0, 0), 0), (ZOMBIE, px + 9, py + 9, 5, (0, 0), 3)]
  return dict(mat=mat, objects=objs, inventory=None)


def cave(area=(64, 64)):
  """World 2: a skeleton cave right beside the spawn point: stone with tunnels of path, skeletons with and without a reload
  count, coal / iron / diamond in the walls; the player keeps the centre but faces left."""
  W, H = area
  px, py = W // 2, H // 2
  mat = np.full((W, H), MAT['stone'], np.uint8)
  mat[px - 9:px + 10, py - 1:py + 2] = MAT['path']
  mat[px - 1:px + 2, py - 9:py + 10] = MAT['path']
  mat[px + 4:px + 9, py + 3:py + 8] = MAT['path']
  mat[px + 6, py + 2] = MAT['path']
  mat[px - 2, py - 3] = MAT['coal']
  mat[px + 2, py + 4] = MAT['iron']
  mat[px - 2, py + 2] = MAT['diamond']
  mat[0:12, 0:12] = MAT['grass']
  objs = [(PLAYER, px, py, 0, (-1, 0), 0), (SKELETON, px + 4, py, 3, (0, 0), 0), (SKELETON, px - 5, py + 1, 3, (0, 0), 2),
          (SKELETON, px, py - 6, 3, (0, 0), 0), (SKELETON, px + 6, py + 5, 3, (0, 0), 0), (COW, 3, 3, 3, (0, 0), 0)]
  return dict(mat=mat, objects=objs, inventory=inventory(wood_pickaxe=1, stone=3, coal=1, iron=1))


WORLDS = (meadow, garden, cave)


@functools.lru_cache(maxsize=None)
def tape(k, steps=T):
  """The action tape of parity case k: a scripted head (what the case is about), then seeded random actions."""
  rs = np.random.RandomState(700 + k)
  a = rs.randint(0, len(ACT), size=steps).astype(np.int32)
  head = {0: ['noop', 'noop', 'make_wood_pickaxe', 'move_down', 'place_plant'],
          1: ['do', 'noop', 'noop', 'noop', 'noop', 'noop', 'noop', 'move_left'],
          2: ['noop', 'do', 'place_stone', 'noop']}.get(k % 3, [])
  for t, name in enumerate(head):
    a[t] = ACT[name]
  a.setflags(write=False)
  return a


class Run:
  """One oracle episode in an authored world: snapshots[t], frames[t] (t = 0: the reset), rewards, dones, balance events."""


@functools.lru_cache(maxsize=None)
def oracle_run(k, seed, area=(64, 64), view=(9, 9), size=(64, 64), steps=T, first_episode=1, length=10000):
  """Case k's world and tape on AuthoredOracle(seed): `first_episode - 1` generated resets first, then the authored one."""
  o = AuthoredOracle(seed=seed, area=area, view=view, size=size, length=length)
  for _ in range(first_episode - 1):
    o.reset()
  o.world = WORLDS[k % 3](area)
  r = Run()
  r.frames = [o.reset()]
  r.snapshots = [o.snapshot()]
  r.rewards, r.dones, r.balance = [], [], []
  for a in tape(k, steps):
    obs, rew, done, _ = o.step(int(a))
    r.frames.append(obs)
    r.snapshots.append(o.snapshot())
    r.rewards.append(rew)
    r.dones.append(bool(done))
    r.balance.append(o.balance_events)
  return r


def bank_of(target, ks, area=(64, 64), validate=True):
  """A WorldBank over the worlds of cases ks."""
  from crafter_amd.worlds import WorldBank
  ws = [WORLDS[k % 3](area) for k in ks]
  inv = [w['inventory'] if w['inventory'] is not None else inventory() for w in ws]
  return WorldBank(target, np.stack([w['mat'] for w in ws]), [w['objects'] for w in ws], inv, validate=validate)


def bad_cases():
  """name -> an edit of the garden world (edited_garden) that the device has to flag: one per rule of the validation."""
  W = H = 64
  def mat_zero(w): w['mat'][5, 5] = 0
  def mat_high(w): w['mat'][63, 63] = len(MAT) + 1
  def bad_type(w): w['objects'].insert(1, (9, 3, 3, 1, (0, 1), 0))
  def zero_type(w): w['objects'].insert(1, (0, 3, 3, 1, (0, 1), 0))
  def outside_x(w): w['objects'].insert(2, (COW, W, 3, 3, (0, 0), 0))
  def outside_y(w): w['objects'].insert(0, (COW, 3, 65535, 3, (0, 0), 0))
  def occupied(w): w['objects'].append((COW,) + tuple(w['objects'][1][1:3]) + (3, (0, 0), 0))
  def on_player(w): w['objects'].insert(0, (ZOMBIE, W // 2, H // 2, 5, (0, 0), 0))
  def late_player(w): w['objects'].insert(2, (PLAYER, 7, 7, 0, (0, 1), 0))
  def arrow_facing(w): w['objects'].insert(3, (ARROW, 40, 40, 0, (1, 1), 0))
  def player_facing(w): w['objects'].insert(0, (PLAYER, 30, 30, 0, (0, 0), 0))
  def big_facing(w): w['objects'].insert(3, (ARROW, 41, 41, 0, (-128, 0), 0))
  return dict(mat_zero=mat_zero, mat_high=mat_high, bad_type=bad_type, zero_type=zero_type, outside_x=outside_x, outside_y=outside_y,
              occupied=occupied, on_player=on_player, late_player=late_player, arrow_facing=arrow_facing, player_facing=player_facing,
              big_facing=big_facing)


def edited_garden(edit):
  w = garden()
  w = dict(mat=w['mat'].astype(np.int64), objects=list(w['objects']), inventory=inventory())
  edit(w)
  return w


def small_world(area):
  """A world for any area: grass, a pond and a wall near the centre, the player moved, creatures of every class around."""
  W, H = area
  px, py = W // 2, H // 2
  mat = np.full((W, H), MAT['grass'], np.uint8)
  mat[px - 4:px - 2, py - 4:py + 4] = MAT['water']
  mat[px + 5, py - 3:py + 4] = MAT['stone']
  mat[px + 2:px + 4, py + 3] = MAT['path']
  mat[W - 1, H - 1] = MAT['tree']
  objs = [(PLAYER, px + 1, py - 1, 0, (1, 0), 0), (ZOMBIE, px + 2, py - 1, 5, (0, 0), 0), (COW, px - 1, py + 2, 3, (0, 0), 0),
          (SKELETON, px + 2, py + 3, 3, (0, 0), 1), (ARROW, px - 1, py - 3, 0, (0, 1), 0), (PLANT, px + 1, py + 5, 1, (0, 0), 301),
          (COW, 1, 1, 3, (0, 0), 0), (COW, W - 2, H - 2, 3, (0, 0), 0)]
  return dict(mat=mat, objects=objs, inventory=inventory(stone=2, wood=1))
