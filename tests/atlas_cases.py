"""TEST INFRASTRUCTURE: the rule-branch atlas -- a bank of tiny authored worlds, each with a scripted tape of at most 64 steps
and a witness: a predicate over the ORACLE's run alone which proves that the branch of objects.py / env.py the case is about
fired.  Random tapes walk the common branches thousands of times and the rare ones never; here every rare one has a case, and
every test that plays a case asserts its witness first, so a case that stops reaching its branch fails instead of passing
vacuously.  Worlds are functions of `area`, laid out around the player's cell (the centre, or a corner for the rim cases), so the
same atlas runs at 64 x 64, 48 x 40 and 256 x 256.  They are sand but for what a case needs: no balance pass spawns anything on
sand, so what happens is the tape's doing.  Every oracle run is computed once per session and never modified.

tests/golden/reference_runs/atlas.npz (tools/make_worlds_golden.py) pins every case to the real reference."""
import copy
import functools

import numpy as np

from crafter_amd import tables
from tests.worlds_ref import AuthoredOracle

RULES = tables.load_rules()
MAT = {n: i + 1 for i, n in enumerate(RULES['materials'])}
ACT = {n: i for i, n in enumerate(RULES['actions'])}
ITEMS = list(RULES['items'])
ACHIEVEMENTS = list(RULES['achievements'])
PLAYER, COW, ZOMBIE, SKELETON, ARROW, PLANT = range(1, 7)
LEFT, RIGHT, UP, DOWN = (-1, 0), (1, 0), (0, -1), (0, 1)
RADIUS = 18   # env.py:88: 2 * max(view), the same for the (9, 9) and the (7, 9) view

# the mutated rule set of the RUL = 0 runs: iron asks for the wood pickaxe only and grass nearly always gives a sapling, which
# changes what `mine` witnesses (iron at step 14) and when `forage` finds its saplings: the standard witness of `mine` must FAIL there
MUTATED_RULES = copy.deepcopy(RULES)
MUTATED_RULES['collect']['iron']['require'] = {'wood_pickaxe': 1}
MUTATED_RULES['collect']['grass']['probability'] = 0.9


def inventory(**kw):
  return [int(kw.get(n, RULES['items'][n]['initial'])) for n in ITEMS]


class World:
  """A sand world under construction; cells and objects are given relative to the origin `o` (the player's cell)."""

  def __init__(self, area, origin=None, facing=DOWN, **inv):
    self.W, self.H = area
    self.o = (self.W // 2, self.H // 2) if origin is None else origin
    self.mat = np.full(area, MAT['sand'], np.uint8)
    self.objects = [(PLAYER, self.o[0], self.o[1], 0, facing, 0)]
    self.inv = inventory(**inv)

  def put(self, name, *cells):
    for dx, dy in cells:
      self.mat[self.o[0] + dx, self.o[1] + dy] = MAT[name]

  def add(self, typ, dx, dy, health, facing=(0, 0), aux=0):
    self.objects.append((typ, self.o[0] + dx, self.o[1] + dy, health, facing, aux))

  def pocket(self, dx, dy, wall='stone', but=()):
    """Walls the four neighbours of (dx, dy) in, but for those listed."""
    self.put(wall, *[(dx + ex, dy + ey) for ex, ey in (LEFT, RIGHT, UP, DOWN) if (ex, ey) not in but])

  def done(self):
    return dict(mat=self.mat, objects=self.objects, inventory=self.inv)


# ------------------------------------------------------------------ reading a run
def inv(s, name):
  return s['inventory'][ITEMS.index(name)]


def ach(s, name):
  return s['achievements'][ACHIEVEMENTS.index(name)]


def objs(s, typ):
  return [o for o in s['objects'] if o[0] == typ]


def player(s):
  return s['objects'][0]


def at(s, x, y):
  return [o for o in s['objects'] if o[1:3] == (x, y)]


def draws(run, t):
  """MT19937 words drawn during step t (1-based; fewer than 624, or nothing could tell)."""
  a, b = run.snapshots[t - 1], run.snapshots[t]
  return (b['mt_pos'] - a['mt_pos']) if np.array_equal(a['mt_key'], b['mt_key']) else b['mt_pos'] + 624 - a['mt_pos']


def same_but_clock(a, b):
  """No item (the four life stats aside, which the clock moves), achievement or cell changed between two snapshots."""
  return a['inventory'][4:] == b['inventory'][4:] and a['achievements'] == b['achievements'] and np.array_equal(a['mat'], b['mat'])


def steps_of(tape, name):
  return [t + 1 for t, a in enumerate(tape) if a == name]


# ------------------------------------------------------------------ the cases: name -> (world(area), tape, witness(run, area))
def mine(area):
  """Coal left, iron right, diamond above, stone below; a table and a furnace on the diagonals; wood for the three pickaxes."""
  w = World(area, wood=3)
  w.put('coal', LEFT), w.put('iron', RIGHT), w.put('diamond', UP), w.put('stone', DOWN)
  w.put('table', (-1, -1)), w.put('furnace', (1, -1))
  return w.done()


MINE_TAPE = ['move_left', 'do', 'move_right', 'do', 'move_up', 'do', 'move_down', 'do',          # 1-8: nothing without a pickaxe
             'make_wood_pickaxe', 'do', 'move_left', 'do', 'move_right', 'do', 'move_up', 'do',  # 10 stone, 12 coal, 14 / 16 still refused
             'make_stone_pickaxe', 'move_right', 'do', 'move_up', 'do',                          # 19 iron, 21 diamond refused
             'make_iron_pickaxe', 'do', 'do']                                                    # 23 diamond; 24: `do` on the path it left


def mine_witness(run, area):
  s = run.snapshots
  px, py = area[0] // 2, area[1] // 2
  assert player(s[24])[1:3] == (px, py), 'the player never leaves the cell'
  for t in (2, 4, 6, 8, 14, 16, 21):
    assert same_but_clock(s[t - 1], s[t]) and draws(run, t) == 0, f'step {t}: a refused collect changes nothing and draws nothing'
  for t, item, cell in ((10, 'stone', DOWN), (12, 'coal', LEFT), (19, 'iron', RIGHT), (23, 'diamond', UP)):
    assert inv(s[t], item) == inv(s[t - 1], item) + 1 and ach(s[t], 'collect_' + item) == 1 and draws(run, t) == 2, (t, item)
    assert s[t - 1]['mat'][px + cell[0], py + cell[1]] == MAT[item] and s[t]['mat'][px + cell[0], py + cell[1]] == MAT['path']
    assert run.rewards[t - 1] == 1.0
  for t, item in ((9, 'wood_pickaxe'), (17, 'stone_pickaxe'), (22, 'iron_pickaxe')):
    assert inv(s[t], item) == 1 and ach(s[t], 'make_' + item) == 1
  assert inv(s[24], 'wood') == 0 and inv(s[24], 'stone') == 0 and same_but_clock(s[23], s[24])


def forage(area):
  """A tree to the left, water to the right, grass below; wood 8 and drink 9 (both clamps); full energy."""
  w = World(area, wood=8, drink=9)
  w.put('tree', LEFT), w.put('water', RIGHT), w.put('grass', DOWN, (0, 2), (1, 1), (-1, 1))
  return w.done()


FORAGE_TAPE = (['sleep', 'move_left', 'do', 'do', 'noop', 'noop', 'move_right', 'do', 'move_down'] + ['do'] * 40 +
               ['place_plant', 'do', 'do'])


def forage_witness(run, area):
  s = run.snapshots
  assert not s[1]['sleeping'] and inv(s[0], 'energy') == 9, 'sleep is refused at full energy'
  assert inv(s[3], 'wood') == 9 and ach(s[3], 'collect_wood') == 1 and run.rewards[2] == 1.0
  px, py = area[0] // 2, area[1] // 2
  assert s[2]['mat'][px - 1, py] == MAT['tree'] and s[3]['mat'][px - 1, py] == MAT['grass'], 'a felled tree leaves grass'
  # (4: `do` on the grass the tree left -- the first sapling try)
  assert s[7]['thirst2'] == 14 and s[8]['thirst2'] == 2 and inv(s[8], 'drink') == 9 and ach(s[8], 'collect_drink') == 1, 'drink: clamp and thirst reset'
  assert run.rewards[7] == 1.0
  tries = [t for t in steps_of(FORAGE_TAPE, 'do') if t == 4 or 10 <= t <= 49]
  got = [t for t in tries if inv(s[t], 'sapling') == inv(s[t - 1], 'sapling') + 1]
  assert all(draws(run, t) == 2 for t in tries) and 1 <= len(got) < len(tries), 'both outcomes of the sapling draw'
  assert [run.rewards[t - 1] for t in got] == [1.0] + [0.0] * (len(got) - 1), 'a reward at the first unlock only'
  assert ach(s[50], 'place_plant') == 1 and len(objs(s[50], PLANT)) == 1 and inv(s[50], 'sapling') == inv(s[49], 'sapling') - 1
  for t in (51, 52):
    assert same_but_clock(s[t - 1], s[t]) and ach(s[t], 'eat_plant') == 0, '`do` on an unripe plant does nothing'
  assert objs(s[52], PLANT)[0][6] == 2


def orchard(area):
  """A plant one tick from ripe in front of the player (food 7: the clamp); plants beside a cow, a zombie and a skeleton, each
  walled in, and a plant alone."""
  w = World(area, food=7)
  w.put('grass', DOWN)
  w.add(PLANT, 0, 1, 1, aux=300)
  for k, typ in enumerate((COW, ZOMBIE, SKELETON)):
    x = -6 + 6 * k
    w.pocket(x, -10, but=[DOWN])
    w.put('grass', (x, -9)), w.pocket(x, -9, but=[UP])
    w.add(typ, x, -10, 3)
    w.add(PLANT, x, -9, 1, aux=5)
  w.put('grass', (8, 3))
  w.add(PLANT, 8, 3, 1, aux=5)
  return w.done()


ORCHARD_TAPE = ['noop', 'do', 'do', 'noop']


def orchard_witness(run, area):
  s = run.snapshots
  px, py = area[0] // 2, area[1] // 2
  assert at(s[0], px, py + 1)[0][6] == 300 and at(s[1], px, py + 1)[0][6] == 301, 'ripe in the first step'
  assert not np.array_equal(run.frames[0], run.frames[1]), 'the ripe sprite'
  assert inv(s[2], 'food') == 9 and ach(s[2], 'eat_plant') == 1 and at(s[2], px, py + 1)[0][6] == 1 and run.rewards[1] == 1.0   # (grown = 0, then the plant's own tick)
  assert same_but_clock(s[2], s[3]) and at(s[3], px, py + 1)[0][6] == 2
  assert len(objs(s[0], PLANT)) == 5 and [o[1:3] for o in objs(s[1], PLANT)] == [(px, py + 1), (px + 8, py + 3)], 'creatures eat their plants'
  assert len(objs(s[4], COW)) == len(objs(s[4], ZOMBIE)) == len(objs(s[4], SKELETON)) == 1


def arena(area):
  """The player faces up between a cow (left), a zombie (right, cooldown 0) and a skeleton (below, health 7), each walled in;
  table and furnace on the lower diagonals, water on the upper ones; an arrow crosses the cell in front of the player over the
  water and ends in a stone wall.  The sword tiers are covered over the three creatures together, not each on each: the zombie
  is struck with no sword, the wood and the stone one (1, 2, 3), the skeleton with the stone and the iron one (3, 5), the cow
  with the iron one alone (its damage table is the zombie's; one blow kills it)."""
  w = World(area, facing=UP, wood=3, stone=1, coal=1, iron=1, food=5)
  w.put('water', (-1, -1), (1, -1)), w.put('table', (-1, 1)), w.put('furnace', (1, 1))
  w.put('stone', (-2, 0), (2, 0), (0, 2), (6, -1))
  w.add(COW, -1, 0, 3), w.add(ZOMBIE, 1, 0, 5), w.add(SKELETON, 0, 1, 7)
  w.add(ARROW, -3, -1, 0, RIGHT)
  return w.done()


ARENA_TAPE = ['noop', 'noop', 'noop', 'do', 'move_right', 'do', 'make_wood_sword', 'do', 'make_stone_sword', 'do',   # zombie: 1, 2, 3
              'move_down', 'do', 'make_iron_sword', 'do', 'move_left', 'do', 'noop', 'noop']                          # skeleton: 3, 5; cow: 5


def arena_witness(run, area):
  s = run.snapshots
  px, py = area[0] // 2, area[1] // 2
  assert inv(s[1], 'health') == 7 and inv(s[7], 'health') == 5 and [inv(s[t], 'health') for t in range(2, 7)] == [7] * 5, 'the zombie hits an awake player for 2, every 6 steps'
  assert [o[6] for t in range(1, 8) for o in objs(s[t], ZOMBIE)] == [5, 4, 3, 2, 1, 0, 5]
  arrow = [objs(s[t], ARROW) for t in range(8)]
  assert arrow[3][0][1:3] == (px, py - 1) and same_but_clock(s[3], s[4]) and arrow[4][0][1:4] == (px + 1, py - 1, 0), '`do` on an arrow does nothing'
  assert s[0]['mat'][px + 1, py - 1] == MAT['water'], 'the arrow flies over water'
  assert arrow[7] and not objs(s[9], ARROW) and s[9]['mat'][px + 6, py - 1] == MAT['stone'], 'the arrow ends at the stone'
  # (a creature struck down leaves in its own update of the same step: the player is first in the list)
  zombie = [objs(s[t], ZOMBIE)[0][3] for t in (5, 6, 8, 9)]
  assert zombie == [5, 4, 2, 2] and ach(s[10], 'defeat_zombie') == 1 and ach(s[9], 'defeat_zombie') == 0 and not objs(s[10], ZOMBIE)
  assert [objs(s[t], SKELETON)[0][3] for t in (11, 12, 13)] == [7, 4, 4] and ach(s[14], 'defeat_skeleton') == 1 and not objs(s[14], SKELETON)
  assert objs(s[15], COW)[0][3] == 3 and ach(s[16], 'eat_cow') == 1 and not objs(s[16], COW)
  assert inv(s[16], 'food') == 9 and s[15]['hunger2'] == 30 and s[16]['hunger2'] == 2, 'eat_cow: food clamp, hunger reset'
  assert [inv(s[18], n) for n in ('wood_sword', 'stone_sword', 'iron_sword', 'wood', 'stone', 'coal', 'iron')] == [1, 1, 1, 0, 0, 0, 0]
  assert all(run.rewards[t - 1] > 0.5 for t in (7, 9, 10, 13, 14, 16)), 'an unlock each (step 7: minus the zombie\'s 0.2)'


def nightmare(area):
  """A walled-in zombie (cooldown 0) beside a tired player who lies down at once: 7 for a sleeper, the hit wakes them, the
  cooldown runs, they lie down again and die in their sleep."""
  w = World(area, energy=3)
  w.pocket(1, 0, but=[LEFT])
  w.add(ZOMBIE, 1, 0, 5)
  return w.done()


NIGHTMARE_TAPE = ['sleep', 'noop', 'noop', 'noop', 'noop', 'sleep', 'noop']


def nightmare_witness(run, area):
  s = run.snapshots
  assert s[1]['sleeping'] and inv(s[1], 'health') == 2, 'a sleeper takes 7'
  assert not s[2]['sleeping'], 'the hit wakes the sleeper'
  assert [objs(s[t], ZOMBIE)[0][6] for t in range(1, 8)] == [5, 4, 3, 2, 1, 0, 5]
  assert s[6]['sleeping'] and inv(s[6], 'health') == 2 and inv(s[7], 'health') == 0
  assert run.dones == [False] * 6 + [True] and abs(run.rewards[6] + 0.2) < 1e-12, 'death by a zombie on a sleeper'


def nap(area):
  """Energy 8, nothing around: asleep at once, the counters at half rate, energy back after eleven steps, awake the step after
  (wake_up), and then sleep is refused."""
  return World(area, energy=8).done()


NAP_TAPE = ['sleep'] + ['noop'] * 12 + ['sleep', 'noop']


def nap_witness(run, area):
  s = run.snapshots
  assert all(s[t]['sleeping'] for t in range(1, 12)) and not s[12]['sleeping'] and ach(s[12], 'wake_up') == 1 and ach(s[11], 'wake_up') == 0
  assert [s[t]['hunger2'] for t in range(0, 12)] == list(range(12)) and s[12]['hunger2'] == 13 and s[3]['thirst2'] == 3, 'half rate asleep'
  assert inv(s[10], 'energy') == 8 and inv(s[11], 'energy') == 9 and s[10]['fatigue2'] == -20 and s[11]['fatigue2'] == 0
  assert not np.array_equal(run.frames[0], run.frames[1]), 'the sleep tint'
  assert run.rewards[11] == 1.0
  assert not s[14]['sleeping'] and not s[15]['sleeping'], 'sleep refused at full energy'


def archery(area):
  """Nobody acts.  Arrows in flight towards the player, a walled-in cow over water, a plant over lava, each other, a table, a
  furnace and a stone; a skeleton four cells below the player behind a water cell, its reload at 12; health 5."""
  w = World(area, health=5)
  w.add(ARROW, -3, 0, 0, RIGHT)                                   # the player, at step 3
  w.pocket(6, -4, but=[LEFT]), w.put('water', (3, -4), (4, -4), (5, -4))
  w.add(COW, 6, -4, 3), w.add(ARROW, 2, -4, 0, RIGHT)             # the cow, over water
  w.put('lava', (3, -8), (4, -8), (5, -8)), w.put('grass', (6, -8))
  w.add(PLANT, 6, -8, 1, aux=9), w.add(ARROW, 2, -8, 0, RIGHT)    # the plant, over lava
  w.add(ARROW, -8, 3, 0, RIGHT), w.add(ARROW, -3, 3, 0, LEFT)     # each other, at step 3; the second flies on into the stone
  w.put('stone', (-12, 3))
  w.put('table', (4, 6)), w.add(ARROW, 1, 6, 0, RIGHT)
  w.put('furnace', (4, 8)), w.add(ARROW, 1, 8, 0, RIGHT)
  w.put('water', (0, 3)), w.pocket(0, 4, but=[UP])
  w.add(SKELETON, 0, 4, 3, aux=12)
  return w.done()


ARCHERY_TAPE = ['noop'] * 64


def archery_witness(run, area):
  s = run.snapshots
  px, py = area[0] // 2, area[1] // 2
  assert inv(s[2], 'health') == 5 and inv(s[3], 'health') == 3 and len(objs(s[3], ARROW)) == len(objs(s[2], ARROW)) - 4, 'step 3: player, table, furnace, arrow'
  assert objs(s[3], COW)[0][3] == 3 and objs(s[4], COW)[0][3] == 1, 'the cow, over water'
  assert at(s[4], px + 6, py - 8) and not at(s[5], px + 6, py - 8), 'the plant, over lava'
  assert at(s[2], px - 6, py + 3)[0][4] == 1 and at(s[2], px - 5, py + 3)[0][4] == -1 and at(s[3], px - 6, py + 3)[0][4] == -1 and not at(s[3], px - 5, py + 3), 'arrow on arrow: the hit one flies on'
  assert at(s[8], px - 11, py + 3) and not objs(s[9], ARROW) and s[9]['mat'][px - 12, py + 3] == MAT['stone'], 'stopped by stone'
  for y, name in ((6, 'table'), (8, 'furnace')):
    assert s[2]['mat'][px + 4, py + y] == MAT[name] and s[3]['mat'][px + 4, py + y] == MAT['path'], name
  # the reload: 12 at the reset, so no shot before step 12 although the player is 4 away all the time (eleven refused tries of
  # probability 1/2 each), shots after it, and never two less than four steps apart
  shots = [t for t in range(1, len(s)) if at(s[t], px, py + 3) and not at(s[t - 1], px, py + 3)]
  assert shots and shots[0] >= 12 and all(b - a >= 4 for a, b in zip(shots, shots[1:])), shots
  assert [objs(s[t], SKELETON)[0][6] for t in (1, 11, shots[0])] == [11, 1, 4]
  end = run.dones.index(True) + 1
  assert inv(s[end], 'health') == 0 and at(s[end - 1], px, py + 1)[0][0] == ARROW and inv(s[end - 1], 'health') <= 2, 'death by an arrow'


def mason(area):
  """Lava to the right (the player faces it), water to the left, grass above the cell above, grass two to the right, a second
  lava cell; stone 7, wood 2, a sapling and a wood pickaxe."""
  w = World(area, facing=RIGHT, stone=7, wood=2, sapling=1, wood_pickaxe=1)
  w.put('lava', RIGHT, (3, -1)), w.put('water', LEFT), w.put('grass', (0, -2), (2, 0))
  return w.done()


MASON_TAPE = ['place_stone', 'do', 'place_stone', 'do', 'move_right', 'move_left', 'place_stone',   # on lava, on path; over the former lava; on water
              'move_up', 'place_stone', 'place_stone', 'move_down', 'place_stone',                  # on grass; refused on stone; on sand
              'move_right', 'place_furnace', 'place_plant', 'place_table', 'do', 'place_furnace',   # furnace on grass; plant, table, furnace refused: the wrong material
              'move_up', 'place_table', 'move_down', 'move_down', 'place_furnace', 'place_stone',   # table on sand; furnace and stone refused: no stone left
              'move_up', 'move_up', 'move_right', 'move_right']                                      # ... and into the second lava cell


def mason_witness(run, area):
  s = run.snapshots
  px, py = area[0] // 2, area[1] // 2
  m = lambda t, dx, dy: {v: k for k, v in MAT.items()}[int(s[t]['mat'][px + dx, py + dy])]
  assert (m(0, 1, 0), m(1, 1, 0), m(2, 1, 0), m(3, 1, 0), m(4, 1, 0)) == ('lava', 'stone', 'path', 'stone', 'path')
  assert player(s[5])[1:3] == (px + 1, py) and inv(s[5], 'health') == 9, 'over the former lava'
  assert (m(6, -1, 0), m(7, -1, 0), m(8, 0, -2), m(9, 0, -2), m(11, 0, 1), m(12, 0, 1)) == ('water', 'stone', 'grass', 'stone', 'sand', 'stone')
  assert [inv(s[t], 'stone') for t in (1, 2, 3, 4, 7, 9, 10, 12)] == [6, 7, 6, 7, 6, 5, 5, 4] and same_but_clock(s[9], s[10]), 'refused on stone'
  assert ach(s[12], 'place_stone') == 5 and [run.rewards[t - 1] for t in (1, 3, 7)] == [1.0, 0.0, 0.0]
  # 13: the player stands on the former lava, facing grass.  14: the furnace goes up there (4 stones)
  assert inv(s[14], 'stone') == 0 and m(14, 2, 0) == 'furnace' and ach(s[14], 'place_furnace') == 1
  assert same_but_clock(s[14], s[15]) and inv(s[15], 'sapling') == 1, 'a plant wants grass'
  assert same_but_clock(s[15], s[16]), 'a table does not go on a furnace'
  assert same_but_clock(s[16], s[17]) and same_but_clock(s[17], s[18]), 'too few stones'
  assert m(20, 1, -2) == 'table' and inv(s[20], 'wood') == 0 and ach(s[20], 'place_table') == 1
  assert player(s[22])[1:3] == (px + 1, py + 1) and same_but_clock(s[22], s[23]) and same_but_clock(s[23], s[24]), 'nothing left to place'
  end = len(MASON_TAPE)
  assert player(s[end])[1:3] == (px + 3, py - 1) and inv(s[end], 'health') == 0 and inv(s[end - 1], 'health') == 9
  assert run.dones == [False] * (end - 1) + [True], 'death by lava'


def garden_plot(area):
  """Place / refuse around a plant: grass in front, a sapling and two wood -- the plant goes in, nothing goes on top of it."""
  w = World(area, sapling=1, wood=4, stone=2)
  w.put('grass', DOWN)
  return w.done()


GARDEN_PLOT_TAPE = ['place_plant', 'place_table', 'place_stone', 'place_plant', 'noop']


def garden_plot_witness(run, area):
  s = run.snapshots
  assert ach(s[1], 'place_plant') == 1 and inv(s[1], 'sapling') == 0 and len(objs(s[1], PLANT)) == 1 and run.rewards[0] == 1.0
  for t in (2, 3, 4):
    assert same_but_clock(s[t - 1], s[t]), 'place refused on an occupied cell'
  assert objs(s[5], PLANT)[0][6] == 4, 'the plant placed in step 1 grows from step 2 on'


def workshop(area):
  """A table two cells left and one up, a furnace three cells left and one down; exactly what the six tools cost.  In place:
  no utility.  One step left: the table but no furnace.  Two steps left: both.  Then again, with empty pockets."""
  w = World(area, wood=6, stone=2, coal=2, iron=2)
  w.put('table', (-2, -1)), w.put('furnace', (-3, 1))
  return w.done()


TOOLS = ['wood_pickaxe', 'stone_pickaxe', 'iron_pickaxe', 'wood_sword', 'stone_sword', 'iron_sword']
WORKSHOP_TAPE = (['make_' + n for n in TOOLS] + ['move_left'] + ['make_' + n for n in TOOLS] + ['move_left', 'make_iron_pickaxe', 'make_iron_sword'] +
                 ['make_' + n for n in TOOLS])


def workshop_witness(run, area):
  s = run.snapshots
  assert same_but_clock(s[0], s[6]), 'no utility nearby'
  tools = lambda t: [inv(s[t], n) for n in TOOLS]
  assert tools(13) == [1, 1, 0, 1, 1, 0] and same_but_clock(s[9], s[10]) and same_but_clock(s[12], s[13]), 'a table but no furnace'
  assert tools(16) == [1] * 6 and [inv(s[16], n) for n in ('wood', 'stone', 'coal', 'iron')] == [0] * 4
  assert same_but_clock(s[16], s[22]) and s[22]['achievements'].count(1) == 6, 'utilities but no items'
  assert [run.rewards[t] for t in (7, 8, 10, 11, 14, 15)] == [1.0] * 6


def famine(area):
  """Health 1, no food: sixteen steps to the grave."""
  return World(area, health=1, food=0).done()


FAMINE_TAPE = ['noop'] * 16


def famine_witness(run, area):
  s = run.snapshots
  assert s[15]['recover2'] == -30 and inv(s[15], 'health') == 1 and inv(s[16], 'health') == 0 and s[16]['recover2'] == 0
  assert run.dones == [False] * 15 + [True] and abs(run.rewards[15] + 0.1) < 1e-12, 'death by starvation'


ZOMBIE_AT = 10   # the rim zombies' distance from the corner: more than 8 (every update is a random_dir), less than RADIUS


def rim(corner):
  """The player in a corner of the map, facing out of it, a table on the inward neighbour along x and wood in the pocket
  (World.nearby is EMPTY at x == 0 or y == 0, engine.py:95-103: only the south-east corner can craft); an arrow leaves through
  each of the corner's two edges; on each of the two edges stands a zombie ZOMBIE_AT cells from the player, stone on its three
  neighbours inside the map: too far to be drawn `toward` the player, each of its updates is one random_dir, a quarter of which
  point out of the map.  The tape's noop tail counts: the zombies try until the balance pass takes them away.  Over the four
  corners every edge has two zombies and two arrows."""
  ox, oy = corner   # the outward unit steps

  def places(area):
    W, H = area
    cx, cy = (0 if ox < 0 else W - 1), (0 if oy < 0 else H - 1)
    return cx, cy, {(cx - ZOMBIE_AT * ox, cy): (0, oy), (cx, cy - ZOMBIE_AT * oy): (ox, 0)}   # zombie cell -> its way out

  def world(area):
    cx, cy, zombies = places(area)
    w = World(area, origin=(cx, cy), facing=(ox, 0), wood=3, stone=2, sapling=1)
    w.put('table', (-ox, 0))
    w.add(ARROW, -4 * ox, -3 * oy, 0, (0, oy))
    w.add(ARROW, -3 * ox, -5 * oy, 0, (ox, 0))
    for (x, y), out in zombies.items():
      w.put('stone', *[(x + ex - cx, y + ey - cy) for ex, ey in (LEFT, RIGHT, UP, DOWN) if (ex, ey) != out])
      w.add(ZOMBIE, x - cx, y - cy, 5)
    return w.done()

  def witness(run, area):
    cx, cy, zombies = places(area)
    s = run.snapshots
    assert player(s[0])[1:3] == (cx, cy)
    for t in range(1, 9):
      assert same_but_clock(s[t - 1], s[t]) and player(s[t])[1:3] == (cx, cy), 'do / place / move out of the map'
    assert player(s[5])[4:6] == (ox, 0) and player(s[6])[4:6] == (0, oy)
    assert [e for e in run.refused_outside if e[1] == PLAYER] == [(5, PLAYER, cx + ox, cy), (6, PLAYER, cx, cy + oy)]
    crafts = cx > 0 and cy > 0
    assert inv(s[9], 'wood_pickaxe') == int(crafts) and ach(s[9], 'make_wood_pickaxe') == int(crafts), 'World.nearby at the rim'
    a = [[o[1:3] for o in objs(s[t], ARROW)] for t in range(7)]
    assert a[3] == [(cx - 4 * ox, cy), (cx, cy - 5 * oy)] and a[4] == [], 'both arrows leave the map in step 4'
    for (x, y), (ex, ey) in zombies.items():
      tries = [e[0] for e in run.refused_outside if e[1:] == (ZOMBIE, x + ex, y + ey)]
      assert tries, f'the zombie at {(x, y)} never tries to leave through its edge'
      for t in tries:
        assert draws(run, t) >= 1 and at(s[t - 1], x, y)[0][0] == ZOMBIE, 'the try is a drawn random_dir of the zombie standing there'
    assert all(o[1:3] in zombies for t in range(len(s)) for o in objs(s[t], ZOMBIE)), 'it tries, and stays: no zombie ever leaves its cell'
    assert len(objs(s[9], ZOMBIE)) == 2 and len(run.refused_outside) >= 4

  tape = ['do', 'place_stone', 'place_table', 'place_plant', 'move_' + ('left' if ox < 0 else 'right'),
          'move_' + ('up' if oy < 0 else 'down'), 'do', 'place_stone', 'make_wood_pickaxe']   # (from step 10 on the balance pass may take a zombie away)
  return world, tape, witness


RADIUS_POINTS = [(d * ex, d * ey) for ex, ey in (LEFT, RIGHT, UP, DOWN) for d in (16, 17, 18, 19)] + \
                [(9, -7), (7, -10), (10, -8), (8, -11), (-9, 7), (-7, 10), (-10, 8), (-8, 11)]
RADIUS_ZOMBIES = [(12, 4), (6, 11), (10, 8), (4, 15), (-12, -4), (-6, -11), (-10, -8), (-4, -15)]


def radius(area):
  """Arrows at L1 distance 16, 17, 18 and 19 from the player to the left, right, above, below and on two diagonals, the ones on the axes
  flying towards the player, the others away; zombies at the same distances to the right and to the left.  The player steps towards
  and away: an object moves in a step exactly if it is nearer than 18 AFTER the player has moved (env.py:87-89)."""
  w = World(area)
  for dx, dy in RADIUS_POINTS:   # on the axes: inwards; on the diagonals: outwards along x, each on a row of its own
    w.add(ARROW, dx, dy, 0, (int(np.sign(dx)), 0) if dx and dy else (-int(np.sign(dx)), -int(np.sign(dy))))
  for dx, dy in RADIUS_ZOMBIES:
    w.add(ZOMBIE, dx, dy, 5)
  return w.done()


RADIUS_TAPE = ['noop', 'move_right', 'move_right', 'move_left', 'move_left', 'move_left', 'move_up', 'move_down', 'move_down']


def radius_witness(run, area):
  s = run.snapshots
  n = 1 + len(RADIUS_POINTS) + len(RADIUS_ZOMBIES)
  seen = set()
  for t in range(1, len(RADIUS_TAPE) + 1):
    assert len(s[t]['objects']) == n, 'nothing may vanish in this case'
    px, py = player(s[t])[1:3]
    for k in range(1, n):
      a, b = s[t - 1]['objects'][k], s[t]['objects'][k]
      d = abs(a[1] - px) + abs(a[2] - py)
      assert (a[1:3] != b[1:3]) == (d < RADIUS), f'step {t} object {k}: distance {d}, {a} -> {b}'
      if t > 1 and d in (RADIUS - 1, RADIUS):
        seen.add((a[0], d, player(s[t])[1:3] != player(s[t - 1])[1:3]))
  for typ in (ARROW, ZOMBIE):
    assert {(typ, RADIUS - 1, True), (typ, RADIUS, True)} <= seen, 'no object at 17 / 18 while the player moves'
  assert [player(s[t])[1:3] for t in (0, 3, 6, 9)] == [(area[0] // 2 + dx, area[1] // 2 + dy) for dx, dy in ((0, 0), (2, 0), (-1, 0), (-1, 1))]


NW, NE, SW, SE = (-1, -1), (1, -1), (-1, 1), (1, 1)
CASES = {
    'mine': (mine, MINE_TAPE, mine_witness),
    'forage': (forage, FORAGE_TAPE, forage_witness),
    'orchard': (orchard, ORCHARD_TAPE, orchard_witness),
    'arena': (arena, ARENA_TAPE, arena_witness),
    'nightmare': (nightmare, NIGHTMARE_TAPE, nightmare_witness),
    'nap': (nap, NAP_TAPE, nap_witness),
    'archery': (archery, ARCHERY_TAPE, archery_witness),
    'mason': (mason, MASON_TAPE, mason_witness),
    'garden_plot': (garden_plot, GARDEN_PLOT_TAPE, garden_plot_witness),
    'workshop': (workshop, WORKSHOP_TAPE, workshop_witness),
    'famine': (famine, FAMINE_TAPE, famine_witness),
    'rim_nw': rim(NW), 'rim_ne': rim(NE), 'rim_sw': rim(SW), 'rim_se': rim(SE),
    'radius': (radius, RADIUS_TAPE, radius_witness),
}
NAMES = list(CASES)
N = len(NAMES)
T = 64
SEEDS = [900 + k for k in range(N)]
FRAME_CASES = ('orchard', 'nap')   # the cases whose point is a sprite: the fixture keeps their frames in full
GEOMETRIES = {
    'default': dict(area=(64, 64), view=(9, 9), size=(64, 64)),
    '48x40': dict(area=(48, 40), view=(9, 9), size=(64, 64)),
    '256': dict(area=(256, 256), view=(9, 9), size=(64, 64)),
    '256-generic': dict(area=(256, 256), view=(7, 9), size=(84, 72)),
}
DEATHS = {'mason': 'lava', 'nightmare': 'zombie', 'archery': 'arrow', 'famine': 'starvation'}


def world(name, area=(64, 64)):
  return CASES[name][0](tuple(area))


@functools.lru_cache(maxsize=None)
def tape(name):
  """The case's action ids, padded with noop to T steps."""
  names = CASES[name][1]
  assert len(names) <= T
  a = np.array([ACT[n] for n in names] + [ACT['noop']] * (T - len(names)), np.int32)
  a.setflags(write=False)
  return a


def tapes():
  """[T, N]: every case's padded tape, one column per case."""
  return np.stack([tape(n) for n in NAMES], 1)


class Run:
  """One oracle episode of a case: snapshots[t], frames[t], semantic[t] (t = 0: the reset), rewards, dones; `steps`: how far
  the case is compared -- the T steps of its padded tape, or up to its first done; refused_outside: (step, type, x, y) of every
  move the oracle saw tried to a cell outside the map."""


@functools.lru_cache(maxsize=None)
def oracle_run(name, geometry='default', mutated=False):
  """Case `name` on AuthoredOracle(SEEDS[case]) for its whole padded tape (stopped at the first done)."""
  g = GEOMETRIES[geometry]
  o = AuthoredOracle(seed=SEEDS[NAMES.index(name)], rules=MUTATED_RULES if mutated else None, **g)
  o.world = world(name, g['area'])
  r = Run()
  r.frames, r.snapshots, r.semantic = [o.reset()], [o.snapshot()], [o.semantic()]
  r.rewards, r.dones = [], []
  for a in tape(name):
    obs, rew, done, _ = o.step(int(a))
    r.frames.append(obs), r.snapshots.append(o.snapshot()), r.semantic.append(o.semantic())
    r.rewards.append(rew), r.dones.append(bool(done))
    if done:
      break
  r.steps = len(r.dones)
  r.refused_outside = list(o.refused_outside)
  return r


def witnessed_run(name, geometry='default', mutated=False):
  """The oracle run, its witness asserted (on the mutated rules: not asserted -- see witness_changes)."""
  r = oracle_run(name, geometry, mutated)
  if not mutated:
    CASES[name][2](r, GEOMETRIES[geometry]['area'])
  return r


def witness_changes(geometry='default'):
  """The cases whose standard witness FAILS on the mutated rule set: what the mutation was chosen for."""
  out = []
  for name in NAMES:
    try:
      CASES[name][2](oracle_run(name, geometry, True), GEOMETRIES[geometry]['area'])
    except AssertionError:
      out.append(name)
  return out


def bank_of(target, area=(64, 64), rules=None, names=None):
  """A WorldBank over the atlas at `area`, world k = case k."""
  from crafter_amd.worlds import WorldBank
  ws = [world(n, area) for n in (names or NAMES)]
  geometry = target if not isinstance(target, dict) else dict(target, rules=rules)
  return WorldBank(geometry, np.stack([w['mat'] for w in ws]), [w['objects'] for w in ws], [w['inventory'] for w in ws])


def union(geometry='default'):
  """-> (achievements reached over the atlas, causes of the deaths it holds), from the oracle alone."""
  reached, deaths = set(), set()
  for name in NAMES:
    r = oracle_run(name, geometry)
    reached |= {ACHIEVEMENTS[i] for i, c in enumerate(r.snapshots[-1]['achievements']) if c}
    if r.dones[-1]:
      assert inv(r.snapshots[-1], 'health') == 0
      deaths.add(DEATHS[name])
  return reached, deaths


# ------------------------------------------------------------------ playing the atlas (CPU harness and device)
def runs(geometry='default', mutated=False):
  """The oracle runs of all cases, in bank order, every witness asserted first."""
  for name in NAMES:
    witnessed_run(name, geometry)
  if mutated:
    assert 'mine' in witness_changes(geometry), 'the mutated rules change no witness'
  return [oracle_run(name, geometry, mutated) for name in NAMES]


def alive(rs, t):
  """The rows still compared at step t (1-based): a case leaves at its first done."""
  return [i for i, r in enumerate(rs) if t <= r.steps]


def assert_step(rs, t, obs=None, reward=None, done=None, snapshot=None, semantic=None, where='', cols=None):
  """Step t (1-based; 0: the reset) of every case still compared against what a batch gave: obs / reward / done / semantic
  indexed by case (or by cols[case]: the compact rows of a subset call), snapshot(case) -> a canonical snapshot."""
  from tests.parity import assert_same
  for i in alive(rs, t):
    r, j, at_ = rs[i], (i if cols is None else cols[i]), f'{where}{NAMES[i]} step {t}'
    if obs is not None:
      assert np.array_equal(obs[j], r.frames[t]), f'{at_}: pixels'
    if t and reward is not None:
      assert reward[j] == np.float32(r.rewards[t - 1]) and bool(done[j]) == r.dones[t - 1], f'{at_}: reward / done'
    if semantic is not None:
      assert np.array_equal(np.asarray(semantic[j]).reshape(r.semantic[t].shape), r.semantic[t]), f'{at_}: semantic'
    if snapshot is not None:
      assert_same(snapshot(i), r.snapshots[t], at_)
