#!/usr/bin/env python3
"""Writes tests/golden/reference_runs/nearby_ref.npz: what the UNTOUCHED reference (imported through oracle/reference_harness.py)
answers to `env._world.nearby(player.pos, d)` for every d of tests/nearby_cases.py DISTANCES and to `World.count(material)` for
every material, at the recorded states of its RUNS -- reset, then every fifth of 60 random steps -- and on poked states: the reset
state of POKE_SEED with the player's record moved to a corner or a cell one or two from the west / north border, where numpy's
slices come out empty, clipped or re-clipped.  Data only: per run the player's cell, whether the player sleeps, the counts, the material sets as bits and the
objects as canonical tuples (type, x, y, health, fx, fy, aux) sorted by cell.  Before it writes, the tool asserts that both an
empty and a re-clipped window occur.  tests/test_nearby_host.py and tests/test_gpu_nearby.py hold the mirror and the device against
the fixture.  Needs the reference tree (CRAFTER_REFERENCE); run where that tree exists:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_nearby_golden.py
"""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.dont_write_bytecode = True

from oracle import reference_harness as rh  # noqa: E402
from tests import nearby_cases as nc  # noqa: E402
from tests.reference_runs import ReferenceSide  # noqa: E402


def observe(env, mat_ids):
  """One recorded state -> (pos, World.count by material id, the material set of each distance as bits, per distance the objects)."""
  world, player = env._world, env._player
  canon = {id(o): t for o, t in zip([o for o in world._objects if o is not None], ReferenceSide(env).objects())}
  pos = (int(player.pos[0]), int(player.pos[1]))
  count = [0] + [int(world.count(name)) for name in nc.MATERIALS]
  mats, objs = [], []
  for d in nc.DISTANCES:
    materials, objects = world.nearby(pos, d)
    mats.append(sum(1 << mat_ids[m] for m in materials))
    objs.append(sorted((canon[id(o)] for o in objects), key=lambda t: (t[1], t[2])))
  return pos, count, mats, objs, int(bool(player.sleeping))


def pack(states):
  rows = [(s, di) + tuple(t) for s, (_, _, _, objs, _) in enumerate(states) for di, group in enumerate(objs) for t in group]
  return dict(pos=np.array([s[0] for s in states], np.int16), count=np.array([s[1] for s in states], np.int32),
              mats=np.array([s[2] for s in states], np.uint32), sleeping=np.array([s[4] for s in states], np.uint8),
              objs=np.array(rows, np.int32).reshape(-1, 9))


def main():
  crafter = rh.load()
  out = {'distances': np.array(nc.DISTANCES, np.int32)}
  empty = reclipped = 0
  mat_ids = {name: i + 1 for i, name in enumerate(nc.MATERIALS)}
  for area, seed in nc.RUNS:
    env = crafter.Env(area=area, seed=seed)
    env.reset()
    states = [observe(env, mat_ids)]
    for t, a in enumerate(nc.tape(seed)):
      env.step(int(a))   # (no reset after a done step: like the reference, the tape plays on)
      if (t + 1) % nc.EVERY == 0:
        states.append(observe(env, mat_ids))
    for k, v in pack(states).items():
      out[f'{nc.run_key(area, seed)}/{k}'] = v
    print(nc.run_key(area, seed), len(states), 'states,', sum(len(g) for s in states for g in s[3]), 'object rows')
  for area in sorted({a for a, _ in nc.RUNS}):
    states = []
    for pos in nc.poke_positions(area):
      env = crafter.Env(area=area, seed=nc.POKE_SEED)
      env.reset()
      world, player = env._world, env._player
      assert world._obj_map[pos] == 0, (area, pos)   # the player's record takes a free cell: no other object is hidden
      world._obj_map[pos] = world._obj_map[tuple(player.pos)]
      world._obj_map[tuple(player.pos)] = 0
      player.pos = np.array(pos)
      states.append(observe(env, mat_ids))
      for d, m in zip(nc.DISTANCES, states[-1][2]):
        (x0, x1), (y0, y1) = nc.numpy_axis(pos[0], d, area[0]), nc.numpy_axis(pos[1], d, area[1])
        assert (m == 0) == (x0 >= x1 or y0 >= y1), (area, pos, d)
        empty += m == 0
        reclipped += m != 0 and (pos[0] - d + area[0] < 0 or pos[1] - d + area[1] < 0)
    for k, v in pack(states).items():
      out[f'{area[0]}x{area[1]}/poke/{k}'] = v
  print('empty windows:', empty, 're-clipped windows:', reclipped)
  assert empty >= 8 and reclipped >= 4
  nc.FIXTURE.parent.mkdir(parents=True, exist_ok=True)
  np.savez_compressed(nc.FIXTURE, **out)
  print(nc.FIXTURE, nc.FIXTURE.stat().st_size, 'bytes')


if __name__ == '__main__':
  main()
