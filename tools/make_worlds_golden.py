#!/usr/bin/env python3
"""Records tests/golden/reference_runs/authored_world.npz from the UNTOUCHED reference (imported through
oracle/reference_harness.py), with its worldgen.generate_world replaced AT RUN TIME by the authored function of
include/crafter_hip.h crafter_reset_worlds: write the map, World.add the objects in order, set the inventory.  Everything
else -- Env.reset around the call, every step -- is the reference's own code.  The fixture is data only: one authored 64 x 64
world (tests/worlds_cases.py meadow), its action tape, the state at the reset and at the end in full, a hash of every state
field and of the frame at every step, and sampled frames in full (day and night).  tests/test_worlds_golden.py replays it
against tests/worlds_ref.py AuthoredOracle, which is what the device code is compared with.  Run where the reference is:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_worlds_golden.py
"""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tools'))
sys.dont_write_bytecode = True

from oracle import reference_harness as rh  # noqa: E402
from make_golden import ref_state, sha  # noqa: E402
from tests import worlds_cases as wc  # noqa: E402

OUT = ROOT / 'tests' / 'golden' / 'reference_runs' / 'authored_world.npz'
CASE, SEED = 0, 31
FIELDS = ('mat', 'objects', 'inventory', 'achievements', 'misc', 'chunk_order', 'mt_key', 'mt_pos')


def authored(crafter, world):
  """-> the function that takes generate_world's place: (world, player) -> None."""
  from crafter import objects as robj

  def generate_world(w, player):
    w._mat_map[:] = world['mat']
    for k, (typ, x, y, health, facing, aux) in enumerate(world['objects']):
      if typ == wc.PLAYER:
        assert k == 0
        if (x, y) != tuple(player.pos):
          w.move(player, (x, y))
        player.facing = tuple(facing)
        continue
      obj = {wc.COW: lambda: robj.Cow(w, (x, y)), wc.ZOMBIE: lambda: robj.Zombie(w, (x, y), player),
             wc.SKELETON: lambda: robj.Skeleton(w, (x, y), player), wc.ARROW: lambda: robj.Arrow(w, (x, y), tuple(facing)),
             wc.PLANT: lambda: robj.Plant(w, (x, y))}[typ]()
      w.add(obj)
      obj.health = health
      if typ == wc.ZOMBIE:
        obj.cooldown = aux
      elif typ == wc.SKELETON:
        obj.reload = aux
      elif typ == wc.PLANT:
        obj.grown = aux
    if world['inventory'] is not None:
      player.inventory = {name: int(v) for name, v in zip(player.inventory, world['inventory'])}
  return generate_world


def main():
  crafter = rh.load()
  from crafter import worldgen
  world = wc.WORLDS[CASE]()
  acts = np.array(wc.tape(CASE), np.int32)
  env = crafter.Env(seed=SEED)
  original = worldgen.generate_world
  worldgen.generate_world = authored(crafter, world)
  try:
    obs = env.reset()
  finally:
    worldgen.generate_world = original
  out = {'seed': np.int64(SEED), 'case': np.int32(CASE), 'actions': acts, 'reset_obs': obs}
  state = ref_state(env)
  for k in FIELDS:
    out['reset_' + k] = state[k]
  hashes = {k: [sha(state[k])] for k in FIELDS}
  rewards, dones, obs_sha, frames, frame_steps = [], [], [sha(obs)], [], []
  for t, a in enumerate(acts):
    obs, reward, done, _ = env.step(int(a))
    rewards.append(reward)
    dones.append(bool(done))
    obs_sha.append(sha(obs))
    state = ref_state(env)
    for k in FIELDS:
      hashes[k].append(sha(state[k]))
    if t % 30 == 0 or (env._step >= 148 and t % 8 == 0):
      frames.append(obs)
      frame_steps.append(t)
  for k in FIELDS:
    out['final_' + k] = state[k]
    out['sha_' + k] = np.array(hashes[k], np.uint64)
  out.update(rewards=np.array(rewards, np.float64), dones=np.array(dones, np.uint8), obs_sha=np.array(obs_sha, np.uint64),
             frames=np.array(frames, np.uint8), frame_steps=np.array(frame_steps, np.int32))
  OUT.parent.mkdir(parents=True, exist_ok=True)
  np.savez_compressed(OUT, **out)
  print(f'{OUT.name}: {len(acts)} steps, {len(frames)} full frames, {OUT.stat().st_size} bytes')


if __name__ == '__main__':
  main()
