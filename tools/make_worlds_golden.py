#!/usr/bin/env python3
"""Records tests/golden/reference_runs/authored_world.npz and atlas.npz from the UNTOUCHED reference (imported through
oracle/reference_harness.py), with its worldgen.generate_world replaced AT RUN TIME by the authored function of
include/crafter_hip.h crafter_reset_worlds: write the map, World.add the objects in order, set the inventory.  Everything
else -- Env.reset around the call, every step -- is the reference's own code.  The fixtures are data only: per authored
64 x 64 world (tests/worlds_cases.py meadow; every case of tests/atlas_cases.py), its action tape, the state at the reset and
at the end in full, a hash of every state field and of the frame at every step, and sampled frames in full (day and night).
tests/test_worlds_golden.py replays it against tests/worlds_ref.py AuthoredOracle, which is what the device code is compared
with (tests/test_atlas_golden.py: the atlas).  Run where the reference is:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_worlds_golden.py [authored_world] [atlas]
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
ATLAS = ROOT / 'tests' / 'golden' / 'reference_runs' / 'atlas.npz'
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


def record(crafter, world, acts, seed, keep_frame, atlas=False):
  """One episode of the reference in `world` along `acts` (atlas: stopped at the first done, with a hash of info['semantic']
  at every step) -> the fixture's arrays: the tape, the reset and final state in full, a hash of every state field and of the
  frame at every step, the frames `keep_frame(t, env)` picks in full."""
  from crafter import worldgen
  env = crafter.Env(seed=seed)
  original = worldgen.generate_world
  worldgen.generate_world = authored(crafter, world)
  try:
    obs = env.reset()
  finally:
    worldgen.generate_world = original
  out = {'actions': acts, 'reset_obs': obs}
  state = ref_state(env)
  for k in FIELDS:
    out['reset_' + k] = state[k]
  hashes = {k: [sha(state[k])] for k in FIELDS}
  rewards, dones, obs_sha, sem_sha, frames, frame_steps = [], [], [sha(obs)], [np.uint64(0)], [], []
  for t, a in enumerate(acts):
    obs, reward, done, info = env.step(int(a))
    rewards.append(reward)
    dones.append(bool(done))
    obs_sha.append(sha(obs))
    sem_sha.append(sha(np.asarray(info['semantic'], np.uint8)))
    state = ref_state(env)
    for k in FIELDS:
      hashes[k].append(sha(state[k]))
    if keep_frame(t, env):
      frames.append(obs)
      frame_steps.append(t)
    if done and atlas:
      break
  for k in FIELDS:
    out['final_' + k] = state[k]
    out['sha_' + k] = np.array(hashes[k], np.uint64)
  out.update(rewards=np.array(rewards, np.float64), dones=np.array(dones, np.uint8), obs_sha=np.array(obs_sha, np.uint64),
             frames=np.array(frames, np.uint8).reshape((-1,) + obs.shape), frame_steps=np.array(frame_steps, np.int32))
  if atlas:
    out['sem_sha'] = np.array(sem_sha, np.uint64)
  return out


def save(path, out):
  path.parent.mkdir(parents=True, exist_ok=True)
  np.savez_compressed(path, **out)
  print(f'{path.name}: {path.stat().st_size} bytes')


def make_authored_world(crafter):
  """authored_world.npz: the meadow through a night, sampled frames of day and night."""
  acts = np.array(wc.tape(CASE), np.int32)
  out = {'seed': np.int64(SEED), 'case': np.int32(CASE)}
  out.update(record(crafter, wc.WORLDS[CASE](), acts, SEED, lambda t, env: t % 30 == 0 or (env._step >= 148 and t % 8 == 0)))
  save(OUT, out)


def make_atlas(crafter):
  """atlas.npz: every case of the rule-branch atlas (tests/atlas_cases.py) at the default geometry, keys '<case>.<array>';
  full frames only for the scripted steps of the cases whose point is a sprite."""
  from tests import atlas_cases as ac
  out = {'names': np.array(ac.NAMES), 'seeds': np.array(ac.SEEDS, np.int64)}
  for name, seed in zip(ac.NAMES, ac.SEEDS):
    acts = np.array(ac.tape(name), np.int32)
    rec = record(crafter, ac.world(name), acts, seed, lambda t, env: name in ac.FRAME_CASES and t < len(ac.CASES[name][1]), atlas=True)
    out.update({f'{name}.{k}': v for k, v in rec.items()})
  save(ATLAS, out)


def main(argv):
  """No argument: both fixtures; otherwise the ones named (authored_world, atlas)."""
  crafter = rh.load()
  for name in argv or ['authored_world', 'atlas']:
    {'authored_world': make_authored_world, 'atlas': make_atlas}[name](crafter)


if __name__ == '__main__':
  main(sys.argv[1:])
