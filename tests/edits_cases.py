"""TEST INFRASTRUCTURE: the worlds, edit schedules, action tapes and oracle runs the edit tests share (CPU harness and GPU).  A
case starts in an authored world (so that every cell an edit names is known), is edited before some of its steps and played
along a tape.  Every oracle run is computed once per session and never modified."""
import functools

import numpy as np

from crafter_amd import abi, edits as E, tables
from tests.edits_ref import EditedOracle

RULES = tables.load_rules()
MAT = {n: i + 1 for i, n in enumerate(RULES['materials'])}
ACT = {n: i for i, n in enumerate(RULES['actions'])}
ITEMS = list(RULES['items'])
ACHS = list(RULES['achievements'])
PLAYER, COW, ZOMBIE, SKELETON, ARROW, PLANT = range(1, 7)
GEO = dict(area=(64, 64), n_daylight=10002, length=10000)
SEEDS = (11, 12, 13)
T = 48   # steps per parity case: the clock edits put every case into the night (daylight < 0.5 from step 148 on)


def inventory(**kw):
  return [int(kw.get(n, RULES['items'][n]['initial'])) for n in ITEMS]


def herds(objs, chunks, per=4):
  """`per` cows in each of `chunks` (chunk coordinates), as the authored-world cases crowd them: more than the balance pass
  tolerates by day (despawns)."""
  for cx, cy in chunks:
    for k in range(per):
      objs.append((COW, 12 * cx + 2 + 2 * k, 12 * cy + 3 + k, 3, (0, 0), 0))


def quarry():
  """Case 0: grass, the player at the centre (32, 32) facing down; herds far away."""
  mat = np.full((64, 64), MAT['grass'], np.uint8)
  mat[20:24, 30] = MAT['tree']
  mat[0:3, 0:5] = MAT['water']
  objs = []
  herds(objs, [(1, 0), (0, 3), (4, 1), (1, 4)])
  return dict(mat=mat, objects=objs, inventory=inventory())


def garden():
  """Case 1: a young plant in front of the player; three cows in chunk (4, 4), whose neighbour (3, 4) nobody has touched."""
  mat = np.full((64, 64), MAT['grass'], np.uint8)
  mat[40:44, 20:24] = MAT['sand']
  objs = [(PLANT, 32, 33, 1, (0, 0), 7), (COW, 50, 50, 3, (0, 0), 0), (COW, 52, 52, 3, (0, 0), 0), (COW, 54, 54, 3, (0, 0), 0)]
  herds(objs, [(1, 0), (0, 3), (4, 1)])
  return dict(mat=mat, objects=objs, inventory=inventory())


def yard():
  """Case 2: grass with a strip of path and a pond; nothing but two herds: every object near the player comes by edit."""
  mat = np.full((64, 64), MAT['grass'], np.uint8)
  mat[26:39, 36] = MAT['path']
  mat[24:27, 24:27] = MAT['water']
  objs = []
  herds(objs, [(4, 0), (0, 4)])
  return dict(mat=mat, objects=objs, inventory=inventory())


WORLDS = (quarry, garden, yard)

# case -> {t: the tape applied before step t + 1} (t = 0: right behind the reset)
SCHEDULES = (
    {0: [E.set_clock(139), E.add('zombie', 33, 32), E.set_cell(32, 33, 'stone'), E.set_item('wood_pickaxe', 1)],
     6: [E.add('zombie', 40, 40, health=2, aux=3), E.set_cell(0, 0, 'lava'), E.set_cell(63, 63, 'table')]},
    {0: [E.set_object(32, 33, aux=400), E.remove(50, 50), E.move(52, 52, 47, 52), E.set_object(54, 54, health=1)],
     4: [E.set_clock(160)],
     9: [E.add('cow', 38, 50), E.move(47, 52, 47, 47)]},
    {0: [E.add('skeleton', 30, 30, aux=2), E.add('arrow', 36, 32, facing=(-1, 0)), E.add('plant', 34, 34), E.add('cow', 31, 33),
         E.set_player(hunger2=49, thirst2=39, fatigue2=10, recover2=-29), E.set_item('sapling', 2), E.set_item('health', 5)],
     4: [E.move(32, 32, 10, 10), E.set_object(10, 10, facing=(1, 0)), E.NOP, E.set_cell(11, 10, 'water')],
     7: [E.set_player(sleeping=1), E.set_clock(150), E.set_item('energy', 3)]},
)
HEADS = (['move_down', 'do', 'move_down', 'noop'],
         ['do', 'noop', 'noop', 'noop', 'move_left'],
         ['noop', 'noop', 'noop', 'noop', 'do', 'noop', 'noop', 'noop'])


def schedule(k, without=None):
  """Case k's schedule; without = (t, position): that op left out (the twin runs of the preconditions)."""
  s = {t: list(ops) for t, ops in SCHEDULES[k].items()}
  if without is not None:
    del s[without[0]][without[1]]
  return s


@functools.lru_cache(maxsize=None)
def tape(k, steps=T):
  """The action tape of case k: a scripted head (what the case is about), then seeded random actions."""
  rs = np.random.RandomState(900 + k)
  a = rs.randint(0, len(ACT), size=steps).astype(np.int32)
  for t, name in enumerate(HEADS[k]):
    a[t] = ACT[name]
  a.setflags(write=False)
  return a


def rows(ops):
  """One tape -> what the device gets: np.int32 [L, 8]."""
  return E.encode(GEO, ops, 1)[0]


class Run:
  """One oracle episode of a case: snapshots[t], frames[t] (t = 0: the reset; frames[t] is the frame step t returned, which an
  edit behind it does not redraw), rewards, dones, balance[t] (events up to and including step t), daylight[t], and
  edited[t] = the snapshot right behind the edit applied before step t + 1."""


@functools.lru_cache(maxsize=None)
def oracle_run(k, seed, without=None, steps=T):
  o = EditedOracle(seed=seed)
  o.world = WORLDS[k]()
  sched = schedule(k, without)
  r = Run()
  r.frames, r.snapshots = [o.reset()], [o.snapshot()]
  r.rewards, r.dones, r.balance, r.daylight, r.edited = [], [], [0], [float(o.daylight)], {}
  acts = tape(k)
  for t in range(steps):
    if t in sched:
      o.edit(rows(sched[t]))
      r.edited[t] = o.snapshot()
    obs, rew, done, _ = o.step(int(acts[t]))
    r.frames.append(obs)
    r.snapshots.append(o.snapshot())
    r.rewards.append(rew)
    r.dones.append(bool(done))
    r.balance.append(o.balance_events)
    r.daylight.append(float(o.daylight))
  return r


def bank_of(target, ks):
  from crafter_amd.worlds import WorldBank
  ws = [WORLDS[k]() for k in ks]
  return WorldBank(target, np.stack([w['mat'] for w in ws]), [w['objects'] for w in ws], [w['inventory'] for w in ws])


def raw(kind, *args):
  """An op as raw words (what a device tensor may hold): no builder, no check."""
  return [kind] + list(args) + [0] * (7 - len(args))


def refusals():
  """name -> one env's tape (np.int32 [L, 8]) for the garden world right behind its reset -- the player at (32, 32), a plant at
  (32, 33), cows at (50, 50), (52, 52), (54, 54) -- one per refusal of include/crafter_hip_edit.h.  Each tape carries good ops
  around the bad one: they must be applied."""
  good_head, good_tail = raw(abi.EDIT_SET_CELL, 5, 5, MAT['sand']), raw(abi.EDIT_SET_ITEM, ITEMS.index('wood'), 3)
  n_mat, n_items = len(MAT), len(ITEMS)
  bad = dict(
      unknown_kind=raw(9), negative_kind=raw(-1), huge_kind=raw(2 ** 31 - 1),
      cell_outside_x=raw(abi.EDIT_SET_CELL, 64, 3, MAT['stone']), cell_outside_y=raw(abi.EDIT_SET_CELL, 3, -1, MAT['stone']),
      cell_far_outside=raw(abi.EDIT_SET_CELL, 2 ** 31 - 1, -2 ** 31, MAT['stone']),
      material_zero=raw(abi.EDIT_SET_CELL, 3, 3, 0), material_high=raw(abi.EDIT_SET_CELL, 3, 3, n_mat + 1),
      material_negative=raw(abi.EDIT_SET_CELL, 3, 3, -5),
      add_none=raw(abi.EDIT_ADD, 0, 20, 20, 1, 0, 0, 0), add_player=raw(abi.EDIT_ADD, PLAYER, 20, 20, 0, 0, 1, 0),
      add_no_class=raw(abi.EDIT_ADD, 7, 20, 20, 1, 0, 0, 0), add_outside=raw(abi.EDIT_ADD, COW, 20, 64, 3, 0, 0, 0),
      add_occupied=raw(abi.EDIT_ADD, ZOMBIE, 50, 50, 5, 0, 0, 0), add_on_player=raw(abi.EDIT_ADD, ZOMBIE, 32, 32, 5, 0, 0, 0),
      add_arrow_facing=raw(abi.EDIT_ADD, ARROW, 20, 20, 0, 1, 1, 0), add_arrow_no_facing=raw(abi.EDIT_ADD, ARROW, 20, 21, 0, 0, 0, 0),
      remove_empty=raw(abi.EDIT_REMOVE, 20, 20), remove_player=raw(abi.EDIT_REMOVE, 32, 32), remove_outside=raw(abi.EDIT_REMOVE, -1, 0),
      move_no_source=raw(abi.EDIT_MOVE, 20, 20, 21, 21), move_source_outside=raw(abi.EDIT_MOVE, 64, 64, 21, 21),
      move_outside=raw(abi.EDIT_MOVE, 50, 50, 50, 64), move_occupied=raw(abi.EDIT_MOVE, 50, 50, 52, 52),
      move_player_occupied=raw(abi.EDIT_MOVE, 32, 32, 32, 33),
      object_empty=raw(abi.EDIT_SET_OBJECT, 20, 20, abi.EDIT_AUX, 0, 0, 0, 5), object_outside=raw(abi.EDIT_SET_OBJECT, 0, 64, abi.EDIT_AUX, 0, 0, 0, 5),
      object_which=raw(abi.EDIT_SET_OBJECT, 32, 33, 8 | abi.EDIT_AUX, 0, 0, 0, 350),
      player_health=raw(abi.EDIT_SET_OBJECT, 32, 32, abi.EDIT_HEALTH | abi.EDIT_FACING, 3, -1, 0, 0),
      player_aux=raw(abi.EDIT_SET_OBJECT, 32, 32, abi.EDIT_AUX, 0, 0, 0, 3),
      player_facing=raw(abi.EDIT_SET_OBJECT, 32, 32, abi.EDIT_FACING, 0, 2, 0, 0),
      item_outside=raw(abi.EDIT_SET_ITEM, n_items, 1), item_negative=raw(abi.EDIT_SET_ITEM, -1, 1),
      item_value_high=raw(abi.EDIT_SET_ITEM, ITEMS.index('stone'), 10), item_value_negative=raw(abi.EDIT_SET_ITEM, ITEMS.index('health'), -3),
      field_outside=raw(abi.EDIT_SET_PLAYER, 5, 0), field_negative=raw(abi.EDIT_SET_PLAYER, -1, 0),
      sleeping_two=raw(abi.EDIT_SET_PLAYER, 0, 2), hunger_high=raw(abi.EDIT_SET_PLAYER, 1, 51), thirst_negative=raw(abi.EDIT_SET_PLAYER, 2, -1),
      fatigue_low=raw(abi.EDIT_SET_PLAYER, 3, -21), recover_high=raw(abi.EDIT_SET_PLAYER, 4, 2 ** 31 - 1),
      clock_negative=raw(abi.EDIT_SET_CLOCK, -1), clock_at_length=raw(abi.EDIT_SET_CLOCK, 10000), clock_huge=raw(abi.EDIT_SET_CLOCK, 2 ** 31 - 1),
  )
  return {name: np.array([good_head, op, good_tail], np.int32) for name, op in bad.items()}


def not_refused():
  """Tapes that look like refusals and are none: a move onto the own cell, a facing for a class that keeps none."""
  return dict(move_in_place=np.array([raw(abi.EDIT_MOVE, 50, 50, 50, 50)], np.int32),
              cow_facing=np.array([raw(abi.EDIT_SET_OBJECT, 50, 50, abi.EDIT_FACING, 0, 1, 0, 0)], np.int32))


def geometry_edits(area):
  """Two tapes for tests/worlds_cases.small_world(area), applied behind the reset and four steps on: the zombie beside the player
  replaced by a cow, an arrow flying at the player, a table under him, cows moved from corner to corner (new chunk keys), a
  skeleton at the rim, the clock put to dusk, the player put to sleep."""
  W, H = area
  px, py = W // 2 + 1, H // 2 - 1   # where small_world puts the player
  first = [E.remove(px + 1, py), E.add('cow', px + 1, py), E.add('arrow', px, py + 4, facing=(0, -1)), E.set_cell(px, py + 1, 'table'),
           E.set_object(px, py + 6, aux=2), E.move(1, 1, W - 1, 0), E.set_item('wood_pickaxe', 1), E.set_clock(140)]
  second = [E.move(W - 1, 0, 0, H - 1), E.add('skeleton', W - 1, H - 2, aux=1), E.set_player(sleeping=1, fatigue2=-3), E.set_cell(0, 0, 'path'),
            E.remove(W - 2, H - 2)]
  return first, second
