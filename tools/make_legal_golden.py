#!/usr/bin/env python3
"""Writes tests/golden/reference_runs/legal_ref.npz: the legal-action mask (include/crafter_hip.h crafter_legal_actions) computed
from the UNTOUCHED reference's own objects (imported through oracle/reference_harness.py) -- world[target], world.nearby,
player.is_free, constants.collect / place / make -- after reset and after every step of the cases of tests/legal_ref.py, and on
its poked edge states.  For every state of the tapes it also records what the reference DOES: a deep copy of the env is stepped
with each action, and one with noop, from the same RNG; the bit is "the player's position changed" for a move and "anything
differs from the noop copy" (map, objects, inventory, achievements, counters, RNG stream) for every other action.  Before it
writes, the tool asserts what the mask means:
    non-move, legal == 0  =>  the step is identical to the noop step
    move                  =>  legal == moved
    non-move, legal == 1  =>  something differs -- except `do` on a creature (the same step's balancing may despawn the zombie
                              that was hit), in at most 1 % of the legal non-move cases
tests/test_legal_host.py holds the oracle's restatement against the fixture.  Needs the reference tree (CRAFTER_REFERENCE); run
where that tree exists:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_legal_golden.py
"""
import copy
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.dont_write_bytecode = True

from oracle import reference_harness as rh  # noqa: E402
from tests import legal_ref as lr  # noqa: E402
from tests import scenarios  # noqa: E402
from tests import symbolic_ref as sr  # noqa: E402

OUT = ROOT / 'tests' / 'golden' / 'reference_runs' / 'legal_ref.npz'
CLASS = {'Player': 1, 'Cow': 2, 'Zombie': 3, 'Skeleton': 4, 'Arrow': 5, 'Plant': 6}


def legal_of(env, constants, robj):
  """The definition from the reference's objects."""
  world, player = env._world, env._player
  target = (player.pos[0] + player.facing[0], player.pos[1] + player.facing[1])
  material, obj = world[target]
  tired = player.inventory['energy'] < constants.items['energy']['max']
  awake = not (player.sleeping and tired)
  has = lambda amounts: all(player.inventory[k] >= v for k, v in amounts.items())
  nearby, _ = world.nearby(player.pos, 1)
  out = np.zeros(len(constants.actions), np.uint8)
  for a, action in enumerate(constants.actions):
    if action == 'noop':
      ok = True
    elif action.startswith('move_'):
      d = dict(left=(-1, 0), right=(1, 0), up=(0, -1), down=(0, 1))[action[5:]]
      ok = awake and bool(player.is_free(player.pos + np.array(d)))
    elif action == 'do' and obj:
      ok = awake and (isinstance(obj, (robj.Zombie, robj.Skeleton, robj.Cow)) or (isinstance(obj, robj.Plant) and bool(obj.ripe)))
    elif action == 'do':
      info = constants.collect.get(material)
      ok = awake and (material == 'water' or bool(info and has(info['require'])))
    elif action == 'sleep':
      ok = not player.sleeping and tired
    elif action.startswith('place_'):
      info = constants.place[action[6:]]
      ok = awake and not obj and material in info['where'] and has(info['uses'])
    else:
      info = constants.make[action[5:]]
      ok = awake and all(u in nearby for u in info['nearby']) and has(info['uses'])
    out[a] = ok
  return out


def target_of(env, constants):
  """(class of the object on target or 0, 1 if it is a ripe plant, sleeping, energy < max)."""
  player = env._player
  _, obj = env._world[(player.pos[0] + player.facing[0], player.pos[1] + player.facing[1])]
  return np.array([CLASS[type(obj).__name__] if obj else 0, int(bool(getattr(obj, 'ripe', False))), int(bool(player.sleeping)),
                   int(player.inventory['energy'] < constants.items['energy']['max'])], np.uint8)


def _canon(v):
  if isinstance(v, np.ndarray):
    return (v.dtype.str, v.shape, v.tobytes())
  if isinstance(v, dict):
    return tuple((k, _canon(x)) for k, x in v.items())
  if isinstance(v, (list, tuple)):
    return tuple(_canon(x) for x in v)
  if isinstance(v, set):
    return tuple(sorted(_canon(x) for x in v))
  if isinstance(v, (bool, int, float, str, type(None), np.generic)):
    return v
  return type(v).__name__   # a creature's reference to the player: the player is compared in its own slot


def signature(env):
  """Everything a step can change: map, objects in slot order with every attribute, the player's inventory, achievements and
  counters, the env's own counters, the chunk table, the RNG stream.  (Not player.action: Env.step overwrites it before anything
  reads it, env.py:89.)"""
  world = env._world
  objs = tuple(None if o is None else (type(o).__name__, _canon({k: v for k, v in vars(o).items() if k not in ('world', 'random', 'action')}))
               for o in world._objects)
  slot = {id(o): i for i, o in enumerate(world._objects) if o is not None}
  chunks = tuple((k, tuple(sorted(slot[id(o)] for o in members))) for k, members in world._chunks.items())
  return (world._mat_map.tobytes(), world._obj_map.tobytes(), objs, chunks, _canon(world.random.get_state()), world.daylight,
          env._step, _canon(env._unlocked), env._last_health)


def behaviour_of(env, moves):
  """-> uint8 [n_actions]: moved (moves) / differs from the noop step (the others)."""
  noop = copy.deepcopy(env)
  noop.step(0)
  base = signature(noop)
  out = np.zeros(len(moves), np.uint8)
  for a, is_move in enumerate(moves):
    twin = copy.deepcopy(env)
    before = tuple(twin._player.pos)
    twin.step(a)
    out[a] = (tuple(twin._player.pos) != before) if is_move else (signature(twin) != base)
  return out


def main():
  crafter = rh.load()
  from crafter import constants, objects as robj
  moves = [a.startswith('move_') for a in constants.actions]
  do = list(constants.actions).index('do')
  out = {}
  counts = dict(illegal=0, illegal_differs=0, moves=0, moves_wrong=0, legal=0, legal_same=0, legal_same_not_creature=0)
  for case in lr.CASES:
    acts, gifts, seed, area, poke = lr.tape(case)
    env = crafter.Env(area=area, seed=seed)
    env.reset()
    rows, targets, behaviour = [], [], []

    def record():
      rows.append(legal_of(env, constants, robj))
      targets.append(target_of(env, constants))
      behaviour.append(behaviour_of(env, moves))
    record()
    for t, a in enumerate(acts):
      for item, amount in gifts.get(t, {}).items():
        env._player.inventory[item] = amount
      if t in poke:
        for obj in env._world.objects:
          if isinstance(obj, robj.Plant):
            obj.grown = sr.RIPE
      env.step(int(a))   # (no reset after a done step: like the reference, the tape plays on)
      record()
    legal, target, differs = np.stack(rows), np.stack(targets), np.stack(behaviour)
    out[f'{case}/meta'] = np.array([seed, len(acts), area[0], area[1]] + list(poke), np.int64)
    out[f'{case}/legal'], out[f'{case}/target'], out[f'{case}/behaviour'] = legal, target, differs
    for a, is_move in enumerate(moves):
      if is_move:
        counts['moves'] += legal.shape[0]
        counts['moves_wrong'] += int((legal[:, a] != differs[:, a]).sum())
      else:
        counts['illegal'] += int((legal[:, a] == 0).sum())
        counts['illegal_differs'] += int(((legal[:, a] == 0) & (differs[:, a] != 0)).sum())
        same = (legal[:, a] == 1) & (differs[:, a] == 0) & (a != 0)
        counts['legal'] += int((legal[:, a] == 1).sum()) - (legal.shape[0] if a == 0 else 0)
        counts['legal_same'] += int(same.sum())
        creature = np.isin(target[:, 0], (CLASS['Cow'], CLASS['Zombie'], CLASS['Skeleton']))
        counts['legal_same_not_creature'] += int((same & ~(creature & (a == do))).sum())
    print(f'{case}: {len(acts)} steps, legal fraction per action {legal.mean(0).round(2).tolist()}')
  # the edge states: observed only
  rows = []
  for edge in lr.edge_states():
    env = crafter.Env(area=lr.EDGE_AREA, seed=lr.EDGE_SEED)
    env.reset()
    world, player = env._world, env._player
    for item, amount in scenarios.RICH.items():
      player.inventory[item] = amount
    world._obj_map[tuple(edge['pos'])] = world._obj_map[tuple(player.pos)]
    if tuple(player.pos) != tuple(edge['pos']):
      world._obj_map[tuple(player.pos)] = 0
    player.pos = np.array(edge['pos'])
    player.facing = tuple(edge['facing'])
    world[edge['table']] = 'table'
    world[edge['furnace']] = 'furnace'
    rows.append(legal_of(env, constants, robj))
  out['edge/legal'] = np.stack(rows)
  out['edge/meta'] = np.array([lr.EDGE_SEED, len(rows)] + list(lr.EDGE_AREA), np.int64)
  print('behaviour:', counts)
  assert counts['illegal_differs'] == 0 and counts['moves_wrong'] == 0, counts
  assert counts['legal_same_not_creature'] == 0 and counts['legal_same'] <= 0.01 * counts['legal'], counts
  out['behaviour_counts'] = np.array([counts[k] for k in sorted(counts)], np.int64)
  OUT.parent.mkdir(parents=True, exist_ok=True)
  np.savez_compressed(OUT, **out)
  print(OUT, OUT.stat().st_size, 'bytes')


if __name__ == '__main__':
  main()
