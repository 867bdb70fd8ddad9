#!/usr/bin/env python3
"""Writes tests/golden/reference_runs/symbolic_ref.npz (beside the other reference runs: every *.npz directly under
tests/golden/ is a replay case of tests/test_golden.py): the symbolic observation (include/crafter_hip.h crafter_symbolic) computed from the
UNTOUCHED reference's own objects (imported through oracle/reference_harness.py) -- info['semantic'], player.pos, every
object's `texture` string, player.inventory, player.facing / .sleeping and _world.daylight -- after reset and after every
step of the cases of tests/symbolic_ref.py.  tests/test_symbolic_host.py holds the oracle's restatement against it.  Needs
the reference tree (CRAFTER_REFERENCE); run where that tree exists:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_symbolic_golden.py
"""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.dont_write_bytecode = True

from oracle import reference_harness as rh  # noqa: E402
from tests import symbolic_ref as sr  # noqa: E402

OUT = ROOT / 'tests' / 'golden' / 'reference_runs' / 'symbolic_ref.npz'
VARIANT = {'player-left': 1, 'player-right': 2, 'player-up': 3, 'player-down': 4, 'player-sleep': 5,
           'arrow-left': 1, 'arrow-right': 2, 'arrow-up': 3, 'arrow-down': 4, 'plant': 0, 'plant-ripe': 1,
           'cow': 0, 'zombie': 0, 'skeleton': 0}


def symbolic_of(env, semantic):
  """Section 1 of the definition from the reference's objects: LocalView's cells (engine.py:165-181), SemanticView's ids."""
  world, player = env._world, env._player
  gw, gh = (int(v) for v in env._local_view._grid)
  W, H = (int(v) for v in world.area)
  px, py = (int(v) for v in player.pos)
  local = np.zeros((2, gw, gh), np.uint8)
  for x in range(gw):
    for y in range(gh):
      wx, wy = px + x - gw // 2, py + y - gh // 2
      if 0 <= wx < W and 0 <= wy < H:
        local[0, x, y] = semantic[wx, wy]
  for obj in world.objects:
    x, y = int(obj.pos[0]) - px + gw // 2, int(obj.pos[1]) - py + gh // 2
    if 0 <= x < gw and 0 <= y < gh:
      local[1, x, y] = VARIANT[obj.texture]
  stats = np.array(list(player.inventory.values()) + [int(player.facing[0]), int(player.facing[1]), int(bool(player.sleeping))],
                   np.float32)
  return local, np.concatenate([stats, np.array([world.daylight], np.float64).astype(np.float32)])


def main():
  crafter = rh.load()
  from crafter import objects as robj
  out = {}
  for case in sr.CASES:
    acts, gifts, seed, area, poke = sr.tape(case)
    env = crafter.Env(area=area, seed=seed)
    env.reset()
    rows = [symbolic_of(env, env._sem_view())]
    for t, a in enumerate(acts):
      for item, amount in gifts.get(t, {}).items():
        env._player.inventory[item] = amount
      if t in poke:
        for obj in env._world.objects:
          if isinstance(obj, robj.Plant):
            obj.grown = sr.RIPE
      info = env.step(int(a))[3]   # (no reset after a done step: like the reference, the tape plays on)
      rows.append(symbolic_of(env, info['semantic']))
    out[f'{case}/meta'] = np.array([seed, len(acts), area[0], area[1]] + list(poke), np.int64)
    out[f'{case}/local'] = np.stack([r[0] for r in rows])
    out[f'{case}/stats'] = np.stack([r[1] for r in rows])
    ids = set(np.unique(out[f'{case}/local'][:, 0]).tolist())
    pairs = {(int(i), int(v)) for i, v in zip(out[f'{case}/local'][:, 0].ravel(), out[f'{case}/local'][:, 1].ravel()) if v}
    print(f'{case}: {len(acts)} steps, ids {sorted(ids)}, (id, variant) pairs {sorted(pairs)}')
  OUT.parent.mkdir(parents=True, exist_ok=True)
  np.savez_compressed(OUT, **out)
  print(OUT, OUT.stat().st_size, 'bytes')


if __name__ == '__main__':
  main()
