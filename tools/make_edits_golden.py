#!/usr/bin/env python3
"""Records tests/golden/reference_runs/edits_<case>.npz from the UNTOUCHED reference (imported through oracle/reference_harness.py): the three
parity cases of tests/edits_cases.py -- an authored world (tools/make_worlds_golden.py's run-time replacement of
worldgen.generate_world), then, between the steps the schedule names, the REFERENCE STATEMENTS include/crafter_hip_edit.h puts
beside each op kind, executed on crafter.Env: `world[x, y] = material`, `world.add(...)`, `world.remove(...)`,
`world.move(...)`, attribute assignments, `player.inventory[...] = ...`, `env._step = ...; env._update_time()`.  The fixtures
are data only: the case's number and seed, the state at the reset and at the end in full, a hash of every state field and of
the frame at every step and right behind every edit -- hashes rather than frames, to keep the files small.
tests/test_edits_golden.py replays them against tests/edits_ref.py EditedOracle, which is what the device code is compared with.
Run where the reference is:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_edits_golden.py
"""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tools'))
sys.dont_write_bytecode = True

from crafter_amd import abi  # noqa: E402
from oracle import reference_harness as rh  # noqa: E402
from make_golden import ref_state, sha  # noqa: E402
from make_worlds_golden import FIELDS, authored, save  # noqa: E402
from tests import edits_cases as ec  # noqa: E402

OUT = ROOT / 'tests' / 'golden' / 'reference_runs'   # (tests/golden/*.npz itself is the list of tests/test_golden.py's cases)


def apply(env, tape):
  """One tape (np.int32 [L, 8], every op valid where it stands) as statements of the reference."""
  from crafter import objects as robj
  w, player = env._world, env._player
  materials = {i: name for name, i in ec.MAT.items()}
  for k, a1, a2, a3, a4, a5, a6, a7 in (tuple(int(v) for v in row) for row in tape):
    if k == abi.EDIT_NOP:
      continue
    elif k == abi.EDIT_SET_CELL:
      w[a1, a2] = materials[a3]
    elif k == abi.EDIT_ADD:
      pos = (a2, a3)
      obj = {ec.COW: lambda: robj.Cow(w, pos), ec.ZOMBIE: lambda: robj.Zombie(w, pos, player),
             ec.SKELETON: lambda: robj.Skeleton(w, pos, player), ec.ARROW: lambda: robj.Arrow(w, pos, (a5, a6)),
             ec.PLANT: lambda: robj.Plant(w, pos)}[a1]()
      w.add(obj)
      obj.health = a4
      if a1 == ec.ZOMBIE:
        obj.cooldown = a7
      elif a1 == ec.SKELETON:
        obj.reload = a7
      elif a1 == ec.PLANT:
        obj.grown = a7
    elif k == abi.EDIT_REMOVE:
      obj = w[a1, a2][1]
      assert obj is not None and obj is not player
      w.remove(obj)
    elif k == abi.EDIT_MOVE:
      obj = w[a1, a2][1]
      assert obj is not None
      w.move(obj, (a3, a4))
    elif k == abi.EDIT_SET_OBJECT:
      obj = w[a1, a2][1]
      assert obj is not None
      if a3 & abi.EDIT_HEALTH:
        obj.health = a4
      if a3 & abi.EDIT_FACING:
        obj.facing = (a5, a6)
      if a3 & abi.EDIT_AUX:
        setattr(obj, {robj.Zombie: 'cooldown', robj.Skeleton: 'reload', robj.Plant: 'grown'}[type(obj)], a7)
    elif k == abi.EDIT_SET_ITEM:
      player.inventory[ec.ITEMS[a1]] = a2
    elif k == abi.EDIT_SET_PLAYER:
      name = abi.EDIT_FIELDS[a1]
      if name == 'sleeping':
        player.sleeping = bool(a2)
      else:
        setattr(player, '_' + name[:-1], a2 / 2)
    elif k == abi.EDIT_SET_CLOCK:
      env._step = a1
      env._update_time()
    else:
      raise AssertionError(k)


def record(crafter, k, seed):
  from crafter import worldgen
  env = crafter.Env(seed=seed)
  original = worldgen.generate_world
  worldgen.generate_world = authored(crafter, ec.WORLDS[k]())
  try:
    obs = env.reset()
  finally:
    worldgen.generate_world = original
  acts = np.array(ec.tape(k), np.int32)
  out = {'case': np.int32(k), 'seed': np.int64(seed), 'actions': acts, 'obs_sha': [sha(obs)]}
  state = ref_state(env)
  for f in FIELDS:
    out['reset_' + f] = state[f]
  hashes = {f: [sha(state[f])] for f in FIELDS}
  edited = {f: [] for f in FIELDS}
  edit_steps, rewards, dones, steps = [], [], [], [0]
  for t, a in enumerate(acts):
    if t in ec.SCHEDULES[k]:
      apply(env, ec.rows(ec.SCHEDULES[k][t]))
      state = ref_state(env)
      edit_steps.append(t)
      for f in FIELDS:
        edited[f].append(sha(state[f]))
    obs, reward, done, _ = env.step(int(a))
    rewards.append(reward)
    dones.append(bool(done))
    steps.append(env._step)
    out['obs_sha'].append(sha(obs))
    state = ref_state(env)
    for f in FIELDS:
      hashes[f].append(sha(state[f]))
  for f in FIELDS:
    out['final_' + f] = state[f]
    out['sha_' + f] = np.array(hashes[f], np.uint64)
    out['edited_sha_' + f] = np.array(edited[f], np.uint64)
  out.update(obs_sha=np.array(out['obs_sha'], np.uint64), rewards=np.array(rewards, np.float64), dones=np.array(dones, np.uint8),
             steps=np.array(steps, np.int32), edit_steps=np.array(edit_steps, np.int32))
  return out


def main():
  crafter = rh.load()
  for k, seed in enumerate(ec.SEEDS):
    save(OUT / f'edits_{k}.npz', record(crafter, k, seed))


if __name__ == '__main__':
  main()
